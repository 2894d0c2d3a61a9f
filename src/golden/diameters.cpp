// Golden model of the bidimensional lesion diameters (nm03/measure.h SliceDiameters) and the extended
// sidecar text. Plain single-threaded code that shares nothing with the K9 kernel's method: the
// lesion by stack flood fill in raster order, the top and bottom lesion pixel of every COLUMN as
// candidates (the kernel takes row extremes; both sets hold every convex-hull vertex), and plain
// double loops over the candidates in (y, x) order, where a strict comparison keeps the first, i.e.
// the lexicographically smallest, of equal pairs and points.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <utility>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"

namespace nm03 {
namespace golden {

SliceDiameters measure_diameters(const std::vector<uint8_t>& dilated, int connectivity, int w, int h) {
  if (connectivity != 4 && connectivity != 8) throw std::invalid_argument("measure_diameters: connectivity must be 4 or 8");
  if (w <= 0 || h <= 0 || dilated.size() != (size_t)w * h) throw std::invalid_argument("measure_diameters: mask must be h × w");
  SliceDiameters r{};
  r.lesion_first[0] = r.lesion_first[1] = -1;
  for (int k = 0; k < 4; ++k) r.major[k] = r.perp[k] = -1;

  // Components in raster order of their first pixel; the first one of the largest area is the lesion.
  std::vector<int32_t> label(dilated.size(), 0);
  std::vector<int32_t> stack;
  static const int dx[8] = {1, -1, 0, 0, 1, 1, -1, -1}, dy[8] = {0, 0, 1, -1, 1, -1, 1, -1};
  const int nn = connectivity == 8 ? 8 : 4;
  int32_t count = 0, lesion = 0, first = -1;
  uint32_t best = 0;
  for (int32_t start = 0; start < (int32_t)dilated.size(); ++start) {
    if (!dilated[(size_t)start] || label[(size_t)start]) continue;
    ++count;
    uint32_t area = 0;
    label[(size_t)start] = count;
    stack.push_back(start);
    while (!stack.empty()) {
      const int32_t p = stack.back();
      stack.pop_back();
      ++area;
      const int x = p % w, y = p / w;
      for (int k = 0; k < nn; ++k) {
        const int xx = x + dx[k], yy = y + dy[k];
        if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;
        const size_t q = (size_t)yy * w + xx;
        if (!dilated[q] || label[q]) continue;
        label[q] = count;
        stack.push_back((int32_t)q);
      }
    }
    if (area > best) best = area, lesion = count, first = start;
  }
  if (lesion == 0) return r;
  r.lesion_px = best;
  r.lesion_first[0] = first % w;
  r.lesion_first[1] = first / w;

  // Candidates: the topmost and the bottommost lesion pixel of every column, as (y, x), sorted.
  std::vector<std::pair<int, int>> cand;
  for (int x = 0; x < w; ++x) {
    int top = -1, bottom = -1;
    for (int y = 0; y < h; ++y)
      if (label[(size_t)y * w + x] == lesion) {
        if (top < 0) top = y;
        bottom = y;
      }
    if (top < 0) continue;
    cand.emplace_back(top, x);
    if (bottom != top) cand.emplace_back(bottom, x);
  }
  std::sort(cand.begin(), cand.end());

  int64_t d2max = -1;
  size_t ia = 0, ib = 0;
  for (size_t i = 0; i < cand.size(); ++i)
    for (size_t j = i; j < cand.size(); ++j) {
      const int64_t ey = cand[j].first - cand[i].first, ex = cand[j].second - cand[i].second;
      const int64_t d2 = ex * ex + ey * ey;
      if (d2 > d2max) d2max = d2, ia = i, ib = j;
    }
  r.major_px2 = (uint32_t)d2max;
  r.major[0] = cand[ia].second, r.major[1] = cand[ia].first;
  r.major[2] = cand[ib].second, r.major[3] = cand[ib].first;

  const int64_t ex = r.major[2] - r.major[0], ey = r.major[3] - r.major[1];
  int64_t pmin = 0, pmax = 0;
  size_t ic = 0, id = 0;
  for (size_t i = 0; i < cand.size(); ++i) {
    const int64_t p = -ey * cand[i].second + ex * cand[i].first;
    if (i == 0 || p < pmin) pmin = p, ic = i;
    if (i == 0 || p > pmax) pmax = p, id = i;
  }
  r.perp_extent = (uint32_t)(pmax - pmin);
  r.perp[0] = cand[ic].second, r.perp[1] = cand[ic].first;
  r.perp[2] = cand[id].second, r.perp[3] = cand[id].first;
  return r;
}

std::string measure_json(const SliceMeasure& m, const SliceDiameters& d, const SliceInput& s, const PipelineParams& p) {
  return measure::to_json(m, d, s.w, s.h, s.spacing_x, s.spacing_y, s.slope, s.intercept, p.apply_rescale,
                          p.measure_connectivity);
}

std::string measure_sidecar(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const SliceInput& s,
                            const PipelineParams& p) {
  if (p.measure_texture) {  // the texture keys after all the others: the text without the flag, then they
    PipelineParams q = p;
    q.measure_texture = false;
    const measure::Glcm tx = measure_texture(dilated, s, p.texture_levels);
    return measure::insert_global_keys(measure_sidecar(dilated, region, s, q),
                                       measure::texture_keys(tx.c.data(), (int)tx.head.levels));
  }
  const SliceMeasure m = measure(dilated, region, s, p.measure_connectivity);
  if (p.measure_intensity) {  // the intensity keys after all the others
    const IntensityStats st = measure_intensity(dilated, s);
    if (!p.measure_diameters)
      return measure::to_json(m, st, s.w, s.h, s.spacing_x, s.spacing_y, s.slope, s.intercept, p.apply_rescale,
                              p.measure_connectivity);
    return measure::to_json(m, measure_diameters(dilated, p.measure_connectivity, s.w, s.h), st, s.w, s.h, s.spacing_x,
                            s.spacing_y, s.slope, s.intercept, p.apply_rescale, p.measure_connectivity);
  }
  if (!p.measure_diameters) return measure_json(m, s, p);
  return measure_json(m, measure_diameters(dilated, p.measure_connectivity, s.w, s.h), s, p);
}

}  // namespace golden

namespace measure {

std::string to_json(const SliceMeasure& m, const SliceDiameters& d, int w, int h, float spacing_x, float spacing_y,
                    float slope, float intercept, bool apply_rescale, int connectivity) {
  std::string s = to_json(m, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity);
  s.resize(s.size() - 2);  // reopen the object: drop "}\n"
  char buf[256];
  std::snprintf(buf, sizeof buf,
                ",\"lesion_px\":%u,\"lesion_first\":[%d,%d],\"major_px2\":%u,\"major\":[%d,%d,%d,%d],\"perp_extent\":%u,"
                "\"perp\":[%d,%d,%d,%d]",
                d.lesion_px, d.lesion_first[0], d.lesion_first[1], d.major_px2, d.major[0], d.major[1], d.major[2], d.major[3],
                d.perp_extent, d.perp[0], d.perp[1], d.perp[2], d.perp[3]);
  s += buf;
  auto put_d = [&](const char* key, bool valid, double v) {
    if (valid)
      std::snprintf(buf, sizeof buf, ",\"%s\":%.9g", key, v);
    else
      std::snprintf(buf, sizeof buf, ",\"%s\":null", key);
    s += buf;
  };
  const bool any = d.lesion_px > 0;
  const double sx = (double)spacing_x, sy = (double)spacing_y;
  const double ux = (double)(d.major[2] - d.major[0]) * sx, uy = (double)(d.major[3] - d.major[1]) * sy;
  const double vx = (double)(d.perp[2] - d.perp[0]) * sx, vy = (double)(d.perp[3] - d.perp[1]) * sy;
  const double major_mm = any ? std::sqrt(ux * ux + uy * uy) : 0.0;
  const double perp_mm = major_mm > 0.0 ? std::fabs(ux * vy - uy * vx) / major_mm : 0.0;
  put_d("major_mm", any, major_mm);
  put_d("perp_mm", any, perp_mm);
  put_d("bidimensional_mm2", any, major_mm * perp_mm);
  put_d("major_angle_deg", any && major_mm > 0.0, std::atan2(uy, ux) * (180.0 / 3.14159265358979323846));
  s += "}\n";
  return s;
}

}  // namespace measure
}  // namespace nm03
