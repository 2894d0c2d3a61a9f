// Golden model of the volume measurements (nm03/measure.h VolumeMeasure, VolumeLesion), the sidecar
// text, and the host run of the K8 and K10 kernels' word arithmetic.
//
// golden::measure_volume is plain per-voxel code that shares nothing with the kernels' algorithm:
// components by stack flood fill, cavities by labelling the COMPLEMENT of the 1-voxel-padded mask at
// the dual connectivity, the Euler number by per-voxel loops over the padded array. It is the oracle
// of every GPU comparison. measure::volume_words is the opposite: the kernels' own per-word functions
// (nm03/volume_measure_core.h) over a plain host array, one word after the other.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"
#include "nm03/volume.h"
#include "nm03/volume_measure_core.h"

namespace nm03 {
namespace golden {

namespace {

// Flood fill every component of `value` voxels (non-zero / zero) in a w × h × d byte volume at 6- or
// 26-connectivity: returns the component count and, in `largest`, the largest voxel count.
uint32_t label_components3d(const std::vector<uint8_t>& vol, int w, int h, int d, bool value, int connectivity,
                            uint64_t* largest) {
  std::vector<uint8_t> seen(vol.size(), 0);
  std::vector<size_t> stack;
  uint32_t count = 0;
  uint64_t best = 0;
  for (size_t start = 0; start < vol.size(); ++start) {
    if ((vol[start] != 0) != value || seen[start]) continue;
    ++count;
    uint64_t vox = 0;
    seen[start] = 1;
    stack.push_back(start);
    while (!stack.empty()) {
      const size_t p = stack.back();
      stack.pop_back();
      ++vox;
      const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w % (size_t)h), z = (int)(p / ((size_t)w * h));
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            const int dist = (dx != 0) + (dy != 0) + (dz != 0);
            if (dist == 0 || (connectivity == 6 && dist != 1)) continue;
            const int xx = x + dx, yy = y + dy, zz = z + dz;
            if (xx < 0 || yy < 0 || zz < 0 || xx >= w || yy >= h || zz >= d) continue;
            const size_t q = ((size_t)zz * h + yy) * w + xx;
            if ((vol[q] != 0) != value || seen[q]) continue;
            seen[q] = 1;
            stack.push_back(q);
          }
    }
    if (vox > best) best = vox;
  }
  if (largest) *largest = best;
  return count;
}

}  // namespace

VolumeMeasure measure_volume(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const VolumeInput& v,
                             int connectivity) {
  if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("measure_volume: connectivity must be 6 or 26");
  const int w = v.w, h = v.h, d = v.d;
  const size_t n = (size_t)w * h * d;
  if (w <= 0 || h <= 0 || d <= 0 || dilated.size() != n || region.size() != n || v.raw.size() != n)
    throw std::invalid_argument("measure_volume: volumes and samples must be d × h × w");
  VolumeMeasure m{};
  for (int k = 0; k < 6; ++k) m.bbox[k] = -1;
  // The 1-voxel-padded mask: every neighbour of a voxel exists.
  const int pw = w + 2, ph = h + 2, pd = d + 2;
  std::vector<uint8_t> padded((size_t)pw * ph * pd, 0);
  auto P = [&](int x, int y, int z) -> uint8_t& { return padded[((size_t)(z + 1) * ph + (y + 1)) * pw + (x + 1)]; };
  bool first = true;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t i = ((size_t)z * h + y) * w + x;
        if (region[i]) ++m.region_vox;
        if (!dilated[i]) continue;
        P(x, y, z) = 1;
        ++m.volume_vox;
        m.sum_x += (uint64_t)x;
        m.sum_y += (uint64_t)y;
        m.sum_z += (uint64_t)z;
        if (first || x < m.bbox[0]) m.bbox[0] = x;
        if (first || y < m.bbox[1]) m.bbox[1] = y;
        if (first || z < m.bbox[2]) m.bbox[2] = z;
        if (first || x > m.bbox[3]) m.bbox[3] = x;
        if (first || y > m.bbox[4]) m.bbox[4] = y;
        if (first || z > m.bbox[5]) m.bbox[5] = z;
        const int32_t s = stored_sample(v.raw[i], (uint8_t)v.type, (uint8_t)v.stored_bits);
        m.raw_sum += s;
        if (first || s < m.raw_min) m.raw_min = s;
        if (first || s > m.raw_max) m.raw_max = s;
        first = false;
      }
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        if (!P(x, y, z)) continue;
        m.faces_x += (uint64_t)(!P(x - 1, y, z)) + (uint64_t)(!P(x + 1, y, z));
        m.faces_y += (uint64_t)(!P(x, y - 1, z)) + (uint64_t)(!P(x, y + 1, z));
        m.faces_z += (uint64_t)(!P(x, y, z - 1)) + (uint64_t)(!P(x, y, z + 1));
      }
  m.components = label_components3d(dilated, w, h, d, true, connectivity, &m.largest_vox);
  // Cavities: background components of the padded mask other than the outer one (the padding shell is
  // background and connected, so exactly one component reaches the frame).
  m.cavities = label_components3d(padded, pw, ph, pd, false, connectivity == 26 ? 6 : 26, nullptr) - 1u;
  // Euler number: pairs, 2×2 windows and 2×2×2 windows of the padded volume, each named by its highest
  // corner (x, y, z) in 0 … w / h / d; counted when any (26) or all (6) of its voxels are set.
  const bool all = connectivity == 6;
  int64_t n2 = 0, n1 = 0, n0 = 0;
  auto counts = [&](std::initializer_list<int> offs, int x, int y, int z) {
    // offs: bit 0 = x − 1, bit 1 = y − 1, bit 2 = z − 1 of each member
    bool any_set = false, all_set = true;
    for (int o : offs) {
      const bool s = P(x - (o & 1), y - ((o >> 1) & 1), z - ((o >> 2) & 1)) != 0;
      any_set |= s;
      all_set &= s;
    }
    return all ? all_set : any_set;
  };
  for (int z = 0; z <= d; ++z)
    for (int y = 0; y <= h; ++y)
      for (int x = 0; x <= w; ++x) {
        n2 += counts({0, 1}, x, y, z) + counts({0, 2}, x, y, z) + counts({0, 4}, x, y, z);
        n1 += counts({0, 1, 2, 3}, x, y, z) + counts({0, 1, 4, 5}, x, y, z) + counts({0, 2, 4, 6}, x, y, z);
        n0 += counts({0, 1, 2, 3, 4, 5, 6, 7}, x, y, z);
      }
  const int64_t n3 = (int64_t)m.volume_vox;
  m.euler = all ? n3 - n2 + n1 - n0 : n0 - n1 + n2 - n3;
  return m;
}

std::string measure_volume_json(const VolumeMeasure& m, const VolumeInput& v, bool apply_rescale, int connectivity) {
  return measure::volume_to_json(m, v.w, v.h, v.d, (double)v.spacing_x, (double)v.spacing_y, v.spacing_z,
                                 v.spacing_z_source, v.slope, v.intercept, apply_rescale, connectivity);
}

std::vector<VolumeLesion> measure_volume_lesions(const std::vector<uint8_t>& dilated, const VolumeInput& v,
                                                 int connectivity, int max_lesions) {
  if (connectivity != 6 && connectivity != 26)
    throw std::invalid_argument("measure_volume_lesions: connectivity must be 6 or 26");
  if (max_lesions < 1 || max_lesions > kMaxVolumeLesions)
    throw std::invalid_argument("measure_volume_lesions: lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  const int w = v.w, h = v.h, d = v.d;
  const size_t n = (size_t)w * h * d;
  if (w <= 0 || h <= 0 || d <= 0 || dilated.size() != n || v.raw.size() != n)
    throw std::invalid_argument("measure_volume_lesions: volume and samples must be d × h × w");
  auto set = [&](int x, int y, int z) {
    return x >= 0 && y >= 0 && z >= 0 && x < w && y < h && z < d && dilated[((size_t)z * h + y) * w + x] != 0;
  };
  std::vector<uint8_t> seen(n, 0);
  std::vector<size_t> stack;
  std::vector<VolumeLesion> all;
  // Raster order of the start voxels = order of the components' first voxels.
  for (size_t start = 0; start < n; ++start) {
    if (!dilated[start] || seen[start]) continue;
    VolumeLesion l{};
    bool first = true;
    seen[start] = 1;
    stack.push_back(start);
    while (!stack.empty()) {
      const size_t p = stack.back();
      stack.pop_back();
      const int x = (int)(p % (size_t)w), y = (int)(p / (size_t)w % (size_t)h), z = (int)(p / ((size_t)w * h));
      if (first) l.first[0] = x, l.first[1] = y, l.first[2] = z;  // the start voxel
      ++l.voxels;
      l.sum_x += (uint64_t)x;
      l.sum_y += (uint64_t)y;
      l.sum_z += (uint64_t)z;
      const int c[3] = {x, y, z};
      for (int k = 0; k < 3; ++k) {
        if (first || c[k] < l.bbox[k]) l.bbox[k] = c[k];
        if (first || c[k] > l.bbox[3 + k]) l.bbox[3 + k] = c[k];
      }
      l.faces_x += (uint64_t)(!set(x - 1, y, z)) + (uint64_t)(!set(x + 1, y, z));
      l.faces_y += (uint64_t)(!set(x, y - 1, z)) + (uint64_t)(!set(x, y + 1, z));
      l.faces_z += (uint64_t)(!set(x, y, z - 1)) + (uint64_t)(!set(x, y, z + 1));
      const int32_t s = stored_sample(v.raw[p], (uint8_t)v.type, (uint8_t)v.stored_bits);
      l.raw_sum += s;
      if (first || s < l.raw_min) l.raw_min = s;
      if (first || s > l.raw_max) l.raw_max = s;
      first = false;
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
    all.push_back(l);
  }
  // `all` is in first-voxel order: a stable sort by size keeps that order among equals.
  std::stable_sort(all.begin(), all.end(), [](const VolumeLesion& a, const VolumeLesion& b) { return a.voxels > b.voxels; });
  if (all.size() > (size_t)max_lesions) all.resize((size_t)max_lesions);
  return all;
}

std::string measure_volume_json(const VolumeMeasure& m, const std::vector<VolumeLesion>& lesions, int max_lesions,
                                const VolumeInput& v, bool apply_rescale, int connectivity) {
  return measure::volume_to_json(m, lesions.data(), (int)lesions.size(), max_lesions, v.w, v.h, v.d, (double)v.spacing_x,
                                 (double)v.spacing_y, v.spacing_z, v.spacing_z_source, v.slope, v.intercept, apply_rescale,
                                 connectivity);
}

}  // namespace golden

namespace measure {

std::string volume_to_json(const VolumeMeasure& m, int w, int h, int d, double sx, double sy, double sz,
                           const std::string& spacing_z_source, float slope, float intercept, bool apply_rescale,
                           int connectivity) {
  char buf[256];
  std::string s;
  auto put_i = [&](const char* key, long long v, bool comma = true) {
    std::snprintf(buf, sizeof buf, "%s\"%s\":%lld", comma ? "," : "", key, v);
    s += buf;
  };
  auto put_u = [&](const char* key, unsigned long long v) {
    std::snprintf(buf, sizeof buf, ",\"%s\":%llu", key, v);
    s += buf;
  };
  auto put_d = [&](const char* key, bool valid, double v) {
    if (valid)
      std::snprintf(buf, sizeof buf, ",\"%s\":%.9g", key, v);
    else
      std::snprintf(buf, sizeof buf, ",\"%s\":null", key);
    s += buf;
  };
  s += "{";
  put_i("width", w, false);
  put_i("height", h);
  put_i("depth", d);
  put_i("connectivity", connectivity);
  put_u("volume_vox", m.volume_vox);
  put_u("region_vox", m.region_vox);
  std::snprintf(buf, sizeof buf, ",\"bbox\":[%d,%d,%d,%d,%d,%d]", m.bbox[0], m.bbox[1], m.bbox[2], m.bbox[3], m.bbox[4],
                m.bbox[5]);
  s += buf;
  put_u("sum_x", m.sum_x);
  put_u("sum_y", m.sum_y);
  put_u("sum_z", m.sum_z);
  put_u("faces_x", m.faces_x);
  put_u("faces_y", m.faces_y);
  put_u("faces_z", m.faces_z);
  put_u("components", m.components);
  put_u("largest_vox", m.largest_vox);
  put_u("cavities", m.cavities);
  put_i("euler", m.euler);
  put_i("raw_sum", m.raw_sum);
  put_i("raw_min", m.raw_min);
  put_i("raw_max", m.raw_max);
  put_i("tunnels", (long long)m.components + (long long)m.cavities - (long long)m.euler);
  put_d("spacing_x", true, sx);
  put_d("spacing_y", true, sy);
  put_d("spacing_z", true, sz);
  s += ",\"spacing_z_source\":\"";
  for (char ch : spacing_z_source)
    if (ch != '"' && ch != '\\' && (unsigned char)ch >= 0x20) s += ch;
  s += "\"";
  const bool any = m.volume_vox > 0;
  const double n = (double)m.volume_vox;
  const double mm3 = n * sx * sy * sz;
  const double cx = any ? (double)m.sum_x / n : 0.0, cy = any ? (double)m.sum_y / n : 0.0,
               cz = any ? (double)m.sum_z / n : 0.0;
  double mean = any ? (double)m.raw_sum / n : 0.0;
  if (apply_rescale) mean = mean * (double)slope + (double)intercept;
  put_d("volume_mm3", true, mm3);
  put_d("volume_ml", true, mm3 / 1000.0);
  put_d("surface_mm2", true,
        (double)m.faces_x * sy * sz + (double)m.faces_y * sx * sz + (double)m.faces_z * sx * sy);
  put_d("centroid_x", any, cx);
  put_d("centroid_y", any, cy);
  put_d("centroid_z", any, cz);
  put_d("centroid_x_mm", any, cx * sx);
  put_d("centroid_y_mm", any, cy * sy);
  put_d("centroid_z_mm", any, cz * sz);
  put_d("mean", any, mean);
  s += "}\n";
  return s;
}

std::string volume_to_json(const VolumeMeasure& m, const VolumeLesion* lesions, int count, int lesions_max, int w, int h,
                           int d, double sx, double sy, double sz, const std::string& spacing_z_source, float slope,
                           float intercept, bool apply_rescale, int connectivity) {
  std::string s = volume_to_json(m, w, h, d, sx, sy, sz, spacing_z_source, slope, intercept, apply_rescale, connectivity);
  s.resize(s.size() - 2);  // the closing brace and the newline: the lesion keys follow `mean`
  char buf[256];
  auto put_u = [&](const char* key, unsigned long long v, bool comma = true) {
    std::snprintf(buf, sizeof buf, "%s\"%s\":%llu", comma ? "," : "", key, v);
    s += buf;
  };
  auto put_i = [&](const char* key, long long v) {
    std::snprintf(buf, sizeof buf, ",\"%s\":%lld", key, v);
    s += buf;
  };
  auto put_d = [&](const char* key, double v) {
    std::snprintf(buf, sizeof buf, ",\"%s\":%.9g", key, v);
    s += buf;
  };
  std::snprintf(buf, sizeof buf, ",\"lesions_max\":%d,\"lesions\":[", lesions_max);
  s += buf;
  for (int i = 0; i < count; ++i) {
    const VolumeLesion& l = lesions[i];
    s += i ? ",{" : "{";
    put_u("voxels", l.voxels, false);
    std::snprintf(buf, sizeof buf, ",\"first\":[%d,%d,%d],\"bbox\":[%d,%d,%d,%d,%d,%d]", l.first[0], l.first[1], l.first[2],
                  l.bbox[0], l.bbox[1], l.bbox[2], l.bbox[3], l.bbox[4], l.bbox[5]);
    s += buf;
    put_u("sum_x", l.sum_x);
    put_u("sum_y", l.sum_y);
    put_u("sum_z", l.sum_z);
    put_u("faces_x", l.faces_x);
    put_u("faces_y", l.faces_y);
    put_u("faces_z", l.faces_z);
    put_i("raw_sum", l.raw_sum);
    put_i("raw_min", l.raw_min);
    put_i("raw_max", l.raw_max);
    // A reported lesion has at least one voxel: no null here.
    const double n = (double)l.voxels;
    const double mm3 = n * sx * sy * sz;
    const double cx = (double)l.sum_x / n, cy = (double)l.sum_y / n, cz = (double)l.sum_z / n;
    double mean = (double)l.raw_sum / n;
    if (apply_rescale) mean = mean * (double)slope + (double)intercept;
    put_d("volume_mm3", mm3);
    put_d("volume_ml", mm3 / 1000.0);
    put_d("surface_mm2", (double)l.faces_x * sy * sz + (double)l.faces_y * sx * sz + (double)l.faces_z * sx * sy);
    put_d("equivalent_diameter_mm", std::cbrt(6.0 * mm3 / 3.14159265358979323846));
    put_d("centroid_x", cx);
    put_d("centroid_y", cy);
    put_d("centroid_z", cz);
    put_d("centroid_x_mm", cx * sx);
    put_d("centroid_y_mm", cy * sy);
    put_d("centroid_z_mm", cz * sz);
    put_d("mean", mean);
    s += "}";
  }
  s += "]}\n";
  return s;
}

namespace {
// The parent store of the host run: a plain array, one thread.
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

VolumeMeasure volume_words(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, size_t raw_plane_stride,
                           int w, int h, int d, int wpr, uint8_t type, uint8_t stored_bits, int connectivity) {
  if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("volume_words: connectivity must be 6 or 26");
  const size_t slots = volume_measure_scratch_words(w, h, d);
  if (slots == 0 || wpr != (w + 63) / 64)
    throw std::invalid_argument("volume_words: (w + 1) * h * d + 1 must stay below 2^32, wpr = ceil(w / 64)");
  using namespace vmcore;
  // Poisoned, as the device scratch is uninitialised: only initialised slots may be read.
  std::vector<uint32_t> scratch(slots, 0xDEADBEEFu);
  HostParents par{scratch.data()};
  const BitVolume M{dilated, w, h, d, wpr, false}, C{dilated, w, h, d, wpr, true};
  auto each_word = [&](auto&& fn) {
    for (int z = 0; z < d; ++z)
      for (int y = 0; y < h; ++y)
        for (int k = 0; k < wpr; ++k) fn(z, y, k);
  };
  WordFigures f;
  int64_t raw_sum = 0;
  int32_t r0 = 0x7FFFFFFF, r1 = (int32_t)0x80000000;
  each_word([&](int z, int y, int k) {
    const uint64_t m = word_figures(M, region, z, y, k, connectivity == 6, f);
    init_runs(M, z, y, k, par);
    for (uint64_t t = m; t; t &= t - 1) {
      const int x = (k << 6) + ctz64(t);
      const int32_t v = stored_sample(raw[(size_t)z * raw_plane_stride + (size_t)y * w + x], type, stored_bits);
      raw_sum += v;
      r0 = v < r0 ? v : r0;
      r1 = v > r1 ? v : r1;
    }
  });
  each_word([&](int z, int y, int k) { unite_word(M, par, z, y, k, connectivity == 26); });
  each_word([&](int z, int y, int k) { compress_runs(M, par, z, y, k); });
  each_word([&](int z, int y, int k) {
    stretch_areas(M, par, z, y, k, [&](uint32_t root, uint32_t len) { par.add(root + 1u, len); });
  });
  uint32_t comps = 0, largest = 0, unused = 0;
  each_word([&](int z, int y, int k) { count_roots(M, par, z, y, k, comps, largest, unused); });
  each_word([&](int z, int y, int k) { init_runs(C, z, y, k, par); });
  each_word([&](int z, int y, int k) { unite_word(C, par, z, y, k, connectivity != 26); });
  each_word([&](int z, int y, int k) { compress_runs(C, par, z, y, k); });
  each_word([&](int z, int y, int k) {
    frame_stretches(C, par, z, y, k, [&](uint32_t root) { par.st(root + 1u, 1u); });
  });
  uint32_t croots = 0, cmax = 0, cavities = 0;
  each_word([&](int z, int y, int k) { count_roots(C, par, z, y, k, croots, cmax, cavities); });
  const bool any = f.vox > 0;
  VolumeMeasure r{};
  r.volume_vox = f.vox;
  r.region_vox = f.region;
  const int32_t lo[3] = {f.x0, f.y0, f.z0}, hi[3] = {f.x1, f.y1, f.z1};
  for (int j = 0; j < 3; ++j) {
    r.bbox[j] = any ? lo[j] : -1;
    r.bbox[3 + j] = any ? hi[j] : -1;
  }
  r.components = comps;
  r.cavities = cavities;
  r.sum_x = f.sum_x, r.sum_y = f.sum_y, r.sum_z = f.sum_z;
  r.faces_x = f.faces_x, r.faces_y = f.faces_y, r.faces_z = f.faces_z;
  r.largest_vox = largest;
  r.euler = euler_from_counts(f.e, f.vox, connectivity);
  r.raw_sum = any ? raw_sum : 0;
  r.raw_min = any ? r0 : 0;
  r.raw_max = any ? r1 : 0;
  return r;
}

int volume_lesions_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d, int wpr,
                         uint8_t type, uint8_t stored_bits, int connectivity, int max_lesions, VolumeLesion* out) {
  if (connectivity != 6 && connectivity != 26)
    throw std::invalid_argument("volume_lesions_words: connectivity must be 6 or 26");
  if (max_lesions < 1 || max_lesions > kMaxVolumeLesions)
    throw std::invalid_argument("volume_lesions_words: lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  const size_t slots = volume_measure_scratch_words(w, h, d);
  if (slots == 0 || wpr != (w + 63) / 64)
    throw std::invalid_argument("volume_lesions_words: (w + 1) * h * d + 1 must stay below 2^32, wpr = ceil(w / 64)");
  using namespace vmcore;
  std::vector<uint32_t> scratch(slots, 0xDEADBEEFu);
  HostParents par{scratch.data()};
  const BitVolume M{dilated, w, h, d, wpr, false};
  auto each_word = [&](auto&& fn) {
    for (int z = 0; z < d; ++z)
      for (int y = 0; y < h; ++y)
        for (int k = 0; k < wpr; ++k) fn(z, y, k);
  };
  // K8's mask pass, up to the state K10 reads.
  each_word([&](int z, int y, int k) { init_runs(M, z, y, k, par); });
  each_word([&](int z, int y, int k) { unite_word(M, par, z, y, k, connectivity == 26); });
  each_word([&](int z, int y, int k) { compress_runs(M, par, z, y, k); });
  each_word([&](int z, int y, int k) {
    stretch_areas(M, par, z, y, k, [&](uint32_t root, uint32_t len) { par.add(root + 1u, len); });
  });
  // candidates + select: every root's key, the max_lesions largest.
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
  // accumulate
  std::vector<LesionFigures> fig((size_t)count);
  std::vector<int64_t> rsum((size_t)count, 0);
  std::vector<int32_t> rmin((size_t)count, 0x7FFFFFFF), rmax((size_t)count, (int32_t)0x80000000);
  each_word([&](int z, int y, int k) {
    const uint64_t m = M.at(z, y, k);
    if (m == 0ull) return;
    const WordFaces wf = word_faces(M, z, y, k, m);
    lesion_stretches(M, par, z, y, k, m, [&](uint32_t root, uint64_t bits) {
      const int idx = find_slot(srt_slot.data(), count, root);
      if (idx < 0) return;
      const size_t r = (size_t)srt_rank[(size_t)idx];
      lesion_bits_figures(z, y, k, wf, bits, fig[r]);
      for (uint64_t t = bits; t; t &= t - 1) {
        const int x = (k << 6) + ctz64(t);
        const int32_t v = stored_sample(raw[(size_t)z * raw_plane_stride + (size_t)y * w + x], type, stored_bits);
        rsum[r] += v;
        rmin[r] = v < rmin[r] ? v : rmin[r];
        rmax[r] = v > rmax[r] ? v : rmax[r];
      }
    });
  });
  // final
  for (int i = 0; i < count; ++i) {
    const LesionFigures& f = fig[(size_t)i];
    VolumeLesion r{};
    r.voxels = f.vox;
    slot_voxel(M, lesion_key_slot(keys[(size_t)i]), r.first);
    r.bbox[0] = f.x0, r.bbox[1] = f.y0, r.bbox[2] = f.z0, r.bbox[3] = f.x1, r.bbox[4] = f.y1, r.bbox[5] = f.z1;
    r.sum_x = f.sum_x, r.sum_y = f.sum_y, r.sum_z = f.sum_z;
    r.faces_x = f.faces_x, r.faces_y = f.faces_y, r.faces_z = f.faces_z;
    r.raw_sum = rsum[(size_t)i];
    r.raw_min = rmin[(size_t)i];
    r.raw_max = rmax[(size_t)i];
    out[i] = r;
  }
  return count;
}

}  // namespace measure
}  // namespace nm03
