// Golden model of the per-lesion lengths (nm03/measure.h VolumeLesionDiameters), and the host run of the
// K13 kernels' logic (nm03/volume_diameters_core.h) on K8's run union-find and K10's selection.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"
#include "nm03/volume_diameters_core.h"
#include "nm03/volume_measure_core.h"

namespace nm03 {

namespace {
void check_common(const char* who, int w, int h, int d, int connectivity, int max_lesions, const uint32_t um[3]) {
  const std::string name(who);
  if (connectivity != 6 && connectivity != 26) throw std::invalid_argument(name + ": connectivity must be 6 or 26");
  if (max_lesions < 1 || max_lesions > kMaxVolumeLesions)
    throw std::invalid_argument(name + ": lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument(name + ": empty volume");
  if (volume_measure_scratch_words(w, h, d) == 0)
    throw std::invalid_argument(name + ": (w + 1) * h * d + 1 must stay below 2^32");
  for (int a = 0; a < 3; ++a)
    if (um[a] < 1u) throw std::invalid_argument(name + ": a spacing must be at least 1 um");
  const std::string ext = measure::volume_diameters_extent_error(w, h, d, um);
  if (!ext.empty()) throw std::invalid_argument(name + ": " + ext);
}
}  // namespace

namespace golden {

std::vector<VolumeLesionDiameters> measure_volume_diameters(const std::vector<uint8_t>& dilated, int w, int h, int d,
                                                            int connectivity, int max_lesions, const uint32_t um[3]) {
  check_common("measure_volume_diameters", w, h, d, connectivity, max_lesions, um);
  const size_t n = (size_t)w * h * d;
  if (dilated.size() != n) throw std::invalid_argument("measure_volume_diameters: volume must be d × h × w");
  auto set = [&](int x, int y, int z) {
    return x >= 0 && y >= 0 && z >= 0 && x < w && y < h && z < d && dilated[((size_t)z * h + y) * w + x] != 0;
  };
  struct Voxel {
    int32_t x, y, z;
  };
  // Flood fill per component from the start voxels in raster order, as measure_volume_lesions.
  std::vector<uint8_t> seen(n, 0);
  std::vector<size_t> stack;
  std::vector<std::vector<Voxel>> all;
  for (size_t start = 0; start < n; ++start) {
    if (!dilated[start] || seen[start]) continue;
    std::vector<Voxel> vox;
    seen[start] = 1;
    stack.push_back(start);
    while (!stack.empty()) {
      const size_t p = stack.back();
      stack.pop_back();
      const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w % (size_t)h), z = (int)(p / ((size_t)w * h));
      vox.push_back(Voxel{x, y, z});
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int dist = (dx != 0) + (dy != 0) + (dz != 0);
            if (dist == 0 || (connectivity == 6 && dist != 1)) continue;
            if (!set(x + dx, y + dy, z + dz)) continue;
            const size_t q = ((size_t)(z + dz) * h + (y + dy)) * w + (x + dx);
            if (seen[q]) continue;
            seen[q] = 1;
            stack.push_back(q);
          }
    }
    all.push_back(std::move(vox));
  }
  std::stable_sort(all.begin(), all.end(),
                   [](const std::vector<Voxel>& a, const std::vector<Voxel>& b) { return a.size() > b.size(); });
  if (all.size() > (size_t)max_lesions) all.resize((size_t)max_lesions);
  auto before = [](const Voxel& a, const Voxel& b) {  // raster (z, y, x)
    return a.z != b.z ? a.z < b.z : (a.y != b.y ? a.y < b.y : a.x < b.x);
  };
  std::vector<VolumeLesionDiameters> out;
  for (std::vector<Voxel>& vox : all) {
    // The reduced set: a voxel whose six face neighbours are all mask lies strictly inside a segment of
    // its lesion along every axis, so it ends no maximal pair and no projection.
    std::vector<Voxel> s;
    if (vox.size() <= 64) s = vox;
    else
      for (const Voxel& v : vox)
        if (!set(v.x - 1, v.y, v.z) || !set(v.x + 1, v.y, v.z) || !set(v.x, v.y - 1, v.z) || !set(v.x, v.y + 1, v.z) ||
            !set(v.x, v.y, v.z - 1) || !set(v.x, v.y, v.z + 1))
          s.push_back(v);
    std::sort(s.begin(), s.end(), before);
    VolumeLesionDiameters r{};
    // In raster order of a, then of b ≥ a: the first pair that reaches a strictly larger value wins a tie.
    bool any3 = false, any2 = false;
    size_t a3 = 0, b3 = 0, a2 = 0, b2 = 0;
    for (size_t i = 0; i < s.size(); ++i)
      for (size_t j = i; j < s.size(); ++j) {
        const int64_t dx = (int64_t)(s[j].x - s[i].x) * um[0], dy = (int64_t)(s[j].y - s[i].y) * um[1],
                      dz = (int64_t)(s[j].z - s[i].z) * um[2];
        const uint64_t dxy = (uint64_t)(dx * dx) + (uint64_t)(dy * dy), d3 = dxy + (uint64_t)(dz * dz);
        if (!any3 || d3 > r.major_um2) r.major_um2 = d3, a3 = i, b3 = j, any3 = true;
        if (s[i].z == s[j].z && (!any2 || dxy > r.axial_um2)) r.axial_um2 = dxy, a2 = i, b2 = j, any2 = true;
      }
    const Voxel &ma = s[a3], &mb = s[b3], &aa = s[a2], &ab = s[b2];
    r.major[0] = ma.x, r.major[1] = ma.y, r.major[2] = ma.z, r.major[3] = mb.x, r.major[4] = mb.y, r.major[5] = mb.z;
    r.axial_z = aa.z;
    r.axial[0] = aa.x, r.axial[1] = aa.y, r.axial[2] = ab.x, r.axial[3] = ab.y;
    const int64_t dx = ab.x - aa.x, dy = ab.y - aa.y;
    bool first = true;
    int64_t pmin = 0, pmax = 0;
    for (const Voxel& v : s) {  // raster order: the first voxel at an end is the smallest (y, x)
      if (v.z != aa.z) continue;
      const int64_t p = -dy * v.x + dx * v.y;
      if (first || p < pmin) pmin = p, r.axial_perp[0] = v.x, r.axial_perp[1] = v.y;
      if (first || p > pmax) pmax = p, r.axial_perp[2] = v.x, r.axial_perp[3] = v.y;
      first = false;
    }
    r.axial_perp_extent = pmax - pmin;
    out.push_back(r);
  }
  return out;
}

}  // namespace golden

namespace measure {

void volume_spacing_um(double spacing_x, double spacing_y, double spacing_z, uint32_t um[3]) {
  const double s[3] = {spacing_x, spacing_y, spacing_z};
  for (int a = 0; a < 3; ++a) {
    const double v = s[a] * 1000.0;
    long long q = std::isfinite(v) && v < 4.0e9 ? std::llround(v) : (v > 0 ? 4000000000ll : 1ll);
    um[a] = (uint32_t)std::max(1ll, q);
  }
}

std::string volume_diameters_extent_error(int w, int h, int d, const uint32_t um[3]) {
  const int a = vdcore::extent_overflow(w, h, d, um);
  if (a < 0) return std::string();
  const int dim[3] = {w, h, d};
  const char* names[3] = {"(w - 1) * ux", "(h - 1) * uy", "(d - 1) * uz"};
  return std::string("the volume is too long to measure in micrometres: ") + names[a] + " = " + std::to_string(dim[a] - 1) +
         " * " + std::to_string(um[a]) + " must stay below 2^31";
}

DiameterLengths diameter_lengths(const VolumeLesionDiameters& r, const uint32_t um[3]) {
  DiameterLengths l;
  const double ra = std::sqrt((double)r.axial_um2);
  l.diameter_3d_mm = std::sqrt((double)r.major_um2) / 1000.0;
  l.axial_major_mm = ra / 1000.0;
  l.axial_perp_mm = r.axial_um2 ? (double)um[0] * (double)um[1] * (double)r.axial_perp_extent / ra / 1000.0 : 0.0;
  l.axial_bidimensional_mm2 = l.axial_major_mm * l.axial_perp_mm;
  return l;
}

std::string insert_diameter_keys(std::string text, const VolumeLesionDiameters* dia, int count, const uint32_t um[3]) {
  const size_t at = text.find(",\"lesions_max\":");
  if (at == std::string::npos) throw std::invalid_argument("insert_diameter_keys: the text has no lesion keys");
  char buf[1024];
  std::snprintf(buf, sizeof buf, ",\"diameters_spacing_um\":[%u,%u,%u]", um[0], um[1], um[2]);
  text.insert(at, buf);
  size_t cur = text.find("\"lesions\":[", at);
  for (int i = 0; i < count; ++i) {
    const size_t mean = cur == std::string::npos ? cur : text.find("\"mean\":", cur);
    const size_t close = mean == std::string::npos ? mean : text.find('}', mean);
    if (close == std::string::npos) throw std::invalid_argument("insert_diameter_keys: fewer lesions in the text than records");
    const VolumeLesionDiameters& r = dia[i];
    const DiameterLengths l = diameter_lengths(r, um);
    std::snprintf(buf, sizeof buf,
                  ",\"major_um2\":%llu,\"major\":[%d,%d,%d,%d,%d,%d],\"axial_z\":%d,\"axial_um2\":%llu,\"axial\":[%d,%d,%d,%d],"
                  "\"axial_perp_extent\":%lld,\"axial_perp\":[%d,%d,%d,%d],\"diameter_3d_mm\":%.9g,\"axial_major_mm\":%.9g,"
                  "\"axial_perp_mm\":%.9g,\"axial_bidimensional_mm2\":%.9g",
                  (unsigned long long)r.major_um2, r.major[0], r.major[1], r.major[2], r.major[3], r.major[4], r.major[5],
                  r.axial_z, (unsigned long long)r.axial_um2, r.axial[0], r.axial[1], r.axial[2], r.axial[3],
                  (long long)r.axial_perp_extent, r.axial_perp[0], r.axial_perp[1], r.axial_perp[2], r.axial_perp[3],
                  l.diameter_3d_mm, l.axial_major_mm, l.axial_perp_mm, l.axial_bidimensional_mm2);
    text.insert(close, buf);
    cur = close + std::strlen(buf) + 1;
  }
  return text;
}

namespace {
struct HostParents {
  uint32_t* p;
  uint32_t ld(uint32_t i) const { return p[i]; }
  void st(uint32_t i, uint32_t v) const { p[i] = v; }
  uint32_t fetch_min(uint32_t i, uint32_t v) const {
    const uint32_t old = p[i];
    if (v < old) p[i] = v;
    return old;
  }
  void add(uint32_t i, uint32_t v) const { p[i] += v; }
};
}  // namespace

int volume_diameters_words(const uint64_t* dilated, int w, int h, int d, int wpr, int connectivity, int max_lesions,
                           const uint32_t um[3], bool brute_force, VolumeLesionDiameters* out, uint64_t* skipped) {
  check_common("volume_diameters_words", w, h, d, connectivity, max_lesions, um);
  if (wpr != (w + 63) / 64) throw std::invalid_argument("volume_diameters_words: wpr must be ceil(w / 64)");
  using namespace vmcore;
  using namespace vdcore;
  std::vector<uint32_t> scratch(volume_measure_scratch_words(w, h, d), 0xDEADBEEFu);
  HostParents par{scratch.data()};
  const BitVolume M{dilated, w, h, d, wpr, false};
  auto each_word = [&](auto&& fn) {
    for (int z = 0; z < d; ++z)
      for (int y = 0; y < h; ++y)
        for (int k = 0; k < wpr; ++k) fn(z, y, k);
  };
  // K8's mask pass and K10's selection, as volume_lesions_words.
  each_word([&](int z, int y, int k) { init_runs(M, z, y, k, par); });
  each_word([&](int z, int y, int k) { unite_word(M, par, z, y, k, connectivity == 26); });
  each_word([&](int z, int y, int k) { compress_runs(M, par, z, y, k); });
  each_word([&](int z, int y, int k) {
    stretch_areas(M, par, z, y, k, [&](uint32_t root, uint32_t len) { par.add(root + 1u, len); });
  });
  std::vector<uint64_t> keys;
  each_word([&](int z, int y, int k) {
    uint64_t roots = root_bits(M, par, z, y, k);
    while (roots) {
      int bit = 0;
      keys.push_back(best_root_key(M, par, z, y, k, roots, bit));
      roots &= ~(1ull << bit);
    }
  });
  std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
  const int count = (int)std::min<size_t>(keys.size(), (size_t)max_lesions);
  std::vector<uint32_t> srt_slot((size_t)count);
  for (int i = 0; i < count; ++i) srt_slot[(size_t)i] = lesion_key_slot(keys[(size_t)i]);
  std::sort(srt_slot.begin(), srt_slot.end());
  std::vector<int> srt_rank((size_t)count);
  for (int i = 0; i < count; ++i)
    srt_rank[(size_t)find_slot(srt_slot.data(), count, lesion_key_slot(keys[(size_t)i]))] = i;
  // rows: the table of row extremes and (K10's accumulate) the bounding boxes, from the in-word stretches.
  std::vector<RowExt> table((size_t)count * h * d, RowExt{kRowNoLo, kRowNoHi});
  std::vector<int32_t> lo((size_t)count * 3, 0x7FFFFFFF), hi((size_t)count * 3, -1);
  each_word([&](int z, int y, int k) {
    const uint64_t m = M.at(z, y, k);
    if (m == 0ull) return;
    lesion_stretches(M, par, z, y, k, m, [&](uint32_t root, uint64_t bits) {
      const int idx = find_slot(srt_slot.data(), count, root);
      if (idx < 0) return;
      const int r = srt_rank[(size_t)idx];
      const int32_t s0 = (k << 6) + ctz64(bits), s1 = (k << 6) + 63 - clz64(bits);
      RowExt& e = table[row_index(r, z, y, h, d)];
      e.lo = std::min(e.lo, s0), e.hi = std::max(e.hi, s1);
      const int32_t c0[3] = {s0, y, z}, c1[3] = {s1, y, z};
      for (int a = 0; a < 3; ++a) lo[(size_t)r * 3 + a] = std::min(lo[(size_t)r * 3 + a], c0[a]), hi[(size_t)r * 3 + a] = std::max(hi[(size_t)r * 3 + a], c1[a]);
    });
  });
  const Grid g{w, h, d, um[0], um[1], um[2]};
  uint64_t nskipped = 0;
  for (int rank = 0; rank < count; ++rank) {
    const Rows rows = rows_of(&lo[(size_t)rank * 3], &hi[(size_t)rank * 3]);
    auto row_ext = [&](int z, int y) { return table[row_index(rank, z, y, h, d)]; };
    // tiles
    const uint32_t nt = rows.tiles();
    std::vector<TileBox> tiles(nt, tile_none());
    for (uint32_t r = 0; r < rows.count(); ++r) {
      int y, z;
      rows.row(r, y, z);
      tile_add(z, y, row_ext(z, y), tiles[r / (uint32_t)kTileRows]);
    }
    // bound
    uint64_t l3 = 0, l2 = 0;
    {
      uint32_t pt[2 * kNumDirs];
      for (int dir = 0; dir < kNumDirs; ++dir) {
        int dx, dy, dz;
        direction(dir, dx, dy, dz);
        Extreme eh = extreme_none(), el = extreme_none();
        for (uint32_t r = 0; r < rows.count(); ++r) {
          int y, z;
          rows.row(r, y, z);
          extreme_row(g, z, y, row_ext(z, y), dx, dy, dz, eh, el);
        }
        pt[2 * dir] = eh.pos, pt[2 * dir + 1] = el.pos;
      }
      for (int i = 0; i < 2 * kNumDirs; ++i)
        for (int j = 0; j < 2 * kNumDirs; ++j) l3 = std::max(l3, extreme_d2(g, pt[i], pt[j], false));
      for (int z = rows.z0; z < rows.z0 + rows.nz; ++z) {
        uint32_t pp[2 * kNumPlaneDirs];
        for (int dir = 0; dir < kNumPlaneDirs; ++dir) {
          int dx, dy, dz;
          direction(dir, dx, dy, dz);
          Extreme eh = extreme_none(), el = extreme_none();
          for (int y = rows.y0; y < rows.y0 + rows.ny; ++y) extreme_row(g, z, y, row_ext(z, y), dx, dy, 0, eh, el);
          pp[2 * dir] = eh.pos, pp[2 * dir + 1] = el.pos;
        }
        for (int i = 0; i < 2 * kNumPlaneDirs; ++i)
          for (int j = i + 1; j < 2 * kNumPlaneDirs; ++j) l2 = std::max(l2, extreme_d2(g, pp[i], pp[j], true));
      }
    }
    if (brute_force) l3 = l2 = 0;
    // pairs
    auto cands_of = [&](uint32_t tile, std::vector<Cand>& c) {
      c.clear();
      for (uint32_t r = tile * (uint32_t)kTileRows; r < std::min(rows.count(), (tile + 1) * (uint32_t)kTileRows); ++r) {
        int y, z;
        rows.row(r, y, z);
        const RowExt e = row_ext(z, y);
        if (e.lo > e.hi) continue;
        c.push_back(g.cand(e.lo, y, z));
        if (e.hi != e.lo) c.push_back(g.cand(e.hi, y, z));
      }
    };
    Best b3 = best_none(), b2 = best_none();
    std::vector<Cand> ca, cb;
    for (uint32_t I = 0; I < nt; ++I)
      for (uint32_t J = I; J < nt; ++J) {
        if (tile_pair_skipped(tiles[I], tiles[J], g, l3, l2)) {
          nskipped += !(tiles[I].x0 > tiles[I].x1 || tiles[J].x0 > tiles[J].x1);
          continue;
        }
        cands_of(I, ca);
        cands_of(J, cb);
        for (const Cand& a : ca)
          for (const Cand& b : cb) pair_update(a, b, b3, b2);
      }
    // final
    VolumeLesionDiameters r{};
    r.major_um2 = b3.d2, r.axial_um2 = b2.d2;
    g.voxel((uint32_t)(b3.key >> 32), r.major[0], r.major[1], r.major[2]);
    g.voxel((uint32_t)b3.key, r.major[3], r.major[4], r.major[5]);
    int32_t za, zb;
    g.voxel((uint32_t)(b2.key >> 32), r.axial[0], r.axial[1], za);
    g.voxel((uint32_t)b2.key, r.axial[2], r.axial[3], zb);
    r.axial_z = za;
    const int32_t dx = r.axial[2] - r.axial[0], dy = r.axial[3] - r.axial[1];
    Extreme eh = extreme_none(), el = extreme_none();
    for (int y = rows.y0; y < rows.y0 + rows.ny; ++y) {
      const RowExt e = row_ext(za, y);
      if (e.lo > e.hi) continue;
      for (int s = 0; s < 2; ++s) {
        const int32_t x = s ? e.hi : e.lo;
        const int64_t p = perp_proj(dx, dy, x, y);
        const Extreme c{p, g.pos(x, y, za)}, n{-p, g.pos(x, y, za)};
        if (extreme_beats(c, eh)) eh = c;
        if (extreme_beats(n, el)) el = n;
      }
    }
    r.axial_perp_extent = eh.proj + el.proj;
    int32_t z;
    g.voxel(el.pos, r.axial_perp[0], r.axial_perp[1], z);
    g.voxel(eh.pos, r.axial_perp[2], r.axial_perp[3], z);
    out[rank] = r;
  }
  if (skipped) *skipped = nskipped;
  return count;
}

}  // namespace measure
}  // namespace nm03
