// Golden model of the per-slice measurements (nm03/measure.h) and the sidecar text. Plain
// single-threaded code that shares nothing with the K7 kernel's algorithm: components by stack
// flood fill, holes by labelling the COMPLEMENT of the 1-pixel-padded mask at the dual connectivity
// (not by the Euler identity, which the tests check against this).
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "nm03/golden.h"
#include "nm03/measure.h"

namespace nm03 {
namespace golden {

namespace {
// Flood fill every component of `value` pixels (non-zero / zero) in a w × h byte image: returns the
// component count and, in `largest`, the largest area.
uint32_t label_components(const std::vector<uint8_t>& img, int w, int h, uint8_t value, int connectivity,
                          uint32_t* largest) {
  std::vector<uint8_t> seen(img.size(), 0);
  std::vector<int32_t> stack;
  uint32_t count = 0, best = 0;
  static const int dx[8] = {1, -1, 0, 0, 1, 1, -1, -1}, dy[8] = {0, 0, 1, -1, 1, -1, 1, -1};
  const int nn = connectivity == 8 ? 8 : 4;
  for (int32_t start = 0; start < (int32_t)img.size(); ++start) {
    if ((img[(size_t)start] != 0) != (value != 0) || seen[(size_t)start]) continue;
    ++count;
    uint32_t area = 0;
    seen[(size_t)start] = 1;
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
        if ((img[q] != 0) != (value != 0) || seen[q]) continue;
        seen[q] = 1;
        stack.push_back((int32_t)q);
      }
    }
    if (area > best) best = area;
  }
  if (largest) *largest = best;
  return count;
}
}  // namespace

SliceMeasure measure(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const SliceInput& s,
                     int connectivity) {
  if (connectivity != 4 && connectivity != 8) throw std::invalid_argument("measure: connectivity must be 4 or 8");
  const int w = s.w, h = s.h;
  const size_t n = (size_t)w * h;
  if (w <= 0 || h <= 0 || dilated.size() != n || region.size() != n || s.raw.size() != n)
    throw std::invalid_argument("measure: planes and samples must be h × w");
  SliceMeasure m{};
  for (int k = 0; k < 4; ++k) m.bbox[k] = -1;
  bool first = true;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t i = (size_t)y * w + x;
      if (region[i]) ++m.region_px;
      if (!dilated[i]) continue;
      ++m.area_px;
      m.sum_x += (uint64_t)x;
      m.sum_y += (uint64_t)y;
      if (first || x < m.bbox[0]) m.bbox[0] = x;
      if (first || y < m.bbox[1]) m.bbox[1] = y;
      if (first || x > m.bbox[2]) m.bbox[2] = x;
      if (first || y > m.bbox[3]) m.bbox[3] = y;
      if (x == 0 || !dilated[i - 1]) ++m.perimeter_edges;
      if (x == w - 1 || !dilated[i + 1]) ++m.perimeter_edges;
      if (y == 0 || !dilated[i - (size_t)w]) ++m.perimeter_edges;
      if (y == h - 1 || !dilated[i + (size_t)w]) ++m.perimeter_edges;
      const int32_t v = stored_sample(s.raw[i], (uint8_t)s.type, (uint8_t)s.stored_bits);
      m.raw_sum += v;
      if (first || v < m.raw_min) m.raw_min = v;
      if (first || v > m.raw_max) m.raw_max = v;
      first = false;
    }
  m.components = label_components(dilated, w, h, 1, connectivity, &m.largest_px);
  // Holes: background components of the padded mask other than the outer one (the padding ring is
  // background and connected, so exactly one component reaches the frame).
  const int pw = w + 2, ph = h + 2;
  std::vector<uint8_t> padded((size_t)pw * ph, 0);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) padded[(size_t)(y + 1) * pw + x + 1] = dilated[(size_t)y * w + x] ? 1 : 0;
  m.holes = label_components(padded, pw, ph, 0, connectivity == 8 ? 4 : 8, nullptr) - 1u;
  return m;
}

std::string measure_json(const SliceMeasure& m, const SliceInput& s, const PipelineParams& p) {
  return measure::to_json(m, s.w, s.h, s.spacing_x, s.spacing_y, s.slope, s.intercept, p.apply_rescale,
                          p.measure_connectivity);
}

}  // namespace golden

namespace measure {

int64_t euler_plane(const uint64_t* plane, int w, int h, int wpr, int connectivity) {
  QuadCounts q;
  for (int y = 0; y <= h; ++y)  // row pair (y − 1, y); rows −1 and h are the padding
    for (int k = 0; k < wpr; ++k) {
      const uint64_t mk = row_word_mask(k, w), mp = k > 0 ? row_word_mask(k - 1, w) : 0ull;
      const uint64_t u = y > 0 ? plane[(size_t)(y - 1) * wpr + k] & mk : 0ull;
      const uint64_t up = y > 0 && k > 0 ? plane[(size_t)(y - 1) * wpr + k - 1] & mp : 0ull;
      const uint64_t l = y < h ? plane[(size_t)y * wpr + k] & mk : 0ull;
      const uint64_t lp = y < h && k > 0 ? plane[(size_t)y * wpr + k - 1] & mp : 0ull;
      quad_word(up, u, lp, l, k == wpr - 1 && (w & 63) == 0, q);
    }
  return euler_from_quads(q, connectivity);
}

std::string to_json(const SliceMeasure& m, int w, int h, float spacing_x, float spacing_y, float slope, float intercept,
                    bool apply_rescale, int connectivity) {
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
  put_i("connectivity", connectivity);
  put_u("area_px", m.area_px);
  put_u("region_px", m.region_px);
  std::snprintf(buf, sizeof buf, ",\"bbox\":[%d,%d,%d,%d]", m.bbox[0], m.bbox[1], m.bbox[2], m.bbox[3]);
  s += buf;
  put_u("sum_x", m.sum_x);
  put_u("sum_y", m.sum_y);
  put_u("perimeter_edges", m.perimeter_edges);
  put_u("components", m.components);
  put_u("largest_px", m.largest_px);
  put_u("holes", m.holes);
  put_i("raw_sum", m.raw_sum);
  put_i("raw_min", m.raw_min);
  put_i("raw_max", m.raw_max);
  const bool any = m.area_px > 0;
  const double a = (double)m.area_px, sx = (double)spacing_x, sy = (double)spacing_y;
  const double cx = any ? (double)m.sum_x / a : 0.0, cy = any ? (double)m.sum_y / a : 0.0;
  double mean = any ? (double)m.raw_sum / a : 0.0;
  if (apply_rescale) mean = mean * (double)slope + (double)intercept;
  put_d("area_mm2", true, a * sx * sy);
  put_d("centroid_x", any, cx);
  put_d("centroid_y", any, cy);
  put_d("centroid_x_mm", any, cx * sx);
  put_d("centroid_y_mm", any, cy * sy);
  put_d("mean", any, mean);
  s += "}\n";
  return s;
}

}  // namespace measure
}  // namespace nm03
