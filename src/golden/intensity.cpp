// Golden model of the first-order intensity statistics (nm03/measure.h IntensityStats), the host
// emulation of the K11 kernels' radix select, and the sidecar text of the record.
//
// golden::measure_intensity is the oracle: collect, std::sort, index. It shares only stored_sample and
// the rank formula with the kernels. measure::intensity_words is the opposite: the kernels' two
// histogram passes (nm03/intensity_core.h) over bit planes, one word after the other, without a GPU.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "nm03/golden.h"
#include "nm03/intensity_core.h"
#include "nm03/measure.h"
#include "nm03/volume.h"

namespace nm03 {
namespace golden {

namespace {
IntensityStats sorted_stats(std::vector<int32_t>& v) {
  IntensityStats r{};
  r.count = (uint64_t)v.size();
  if (v.empty()) return r;
  std::sort(v.begin(), v.end());
  for (int32_t s : v) r.sum_sq += (uint64_t)((int64_t)s * (int64_t)s);
  for (int j = 0; j < icore::kPercentiles; ++j)
    r.pct[j] = v[(size_t)(icore::percentile_rank(icore::percentile_of(j), r.count) - 1)];
  return r;
}

IntensityStats collect(const std::vector<uint8_t>& dilated, const std::vector<uint16_t>& raw, size_t n, PixelType type,
                       int stored_bits) {
  if (dilated.size() != n || raw.size() != n) throw std::invalid_argument("measure_intensity: mask and samples must have one shape");
  if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("measure_intensity: stored bits must be 1..16");
  std::vector<int32_t> v;
  for (size_t i = 0; i < n; ++i)
    if (dilated[i]) v.push_back(stored_sample(raw[i], (uint8_t)type, (uint8_t)stored_bits));
  return sorted_stats(v);
}
}  // namespace

IntensityStats measure_intensity(const std::vector<uint8_t>& dilated, const SliceInput& s) {
  if (s.w <= 0 || s.h <= 0) throw std::invalid_argument("measure_intensity: empty slice");
  return collect(dilated, s.raw, (size_t)s.w * s.h, s.type, s.stored_bits);
}

IntensityStats measure_intensity(const std::vector<uint8_t>& dilated, const VolumeInput& v) {
  if (v.w <= 0 || v.h <= 0 || v.d <= 0) throw std::invalid_argument("measure_intensity: empty volume");
  return collect(dilated, v.raw, (size_t)v.w * v.h * v.d, v.type, v.stored_bits);
}

std::string measure_volume_json(const VolumeMeasure& m, const IntensityStats& st, const std::vector<VolumeLesion>* lesions,
                                int max_lesions, const VolumeInput& v, bool apply_rescale, int connectivity) {
  if (lesions)
    return measure::volume_to_json(m, st, lesions->data(), (int)lesions->size(), max_lesions, v.w, v.h, v.d,
                                   (double)v.spacing_x, (double)v.spacing_y, v.spacing_z, v.spacing_z_source, v.slope,
                                   v.intercept, apply_rescale, connectivity);
  return measure::volume_to_json(m, st, v.w, v.h, v.d, (double)v.spacing_x, (double)v.spacing_y, v.spacing_z,
                                 v.spacing_z_source, v.slope, v.intercept, apply_rescale, connectivity);
}

}  // namespace golden

namespace measure {

IntensityStats intensity_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                               int wpr, uint8_t type, uint8_t stored_bits) {
  if (w <= 0 || h <= 0 || d <= 0 || wpr < (w + 63) / 64) throw std::invalid_argument("intensity_words: bad shape");
  // One walk of the set bits, word by word, as the kernels' passes make it.
  auto walk = [&](auto&& f) {
    for (int z = 0; z < d; ++z)
      for (int y = 0; y < h; ++y)
        for (int k = 0; k < (w + 63) / 64; ++k) {
          const uint64_t m = dilated[((size_t)z * h + y) * wpr + k] & row_word_mask(k, w);
          const uint16_t* px = raw + (size_t)z * raw_plane_stride + (size_t)y * w + ((size_t)k << 6);
          for (uint64_t t = m; t; t &= t - 1) {
            const int32_t v = stored_sample(px[__builtin_ctzll(t)], type, stored_bits);
            f(v, (uint32_t)icore::sample_key(v, type));
          }
        }
  };
  IntensityStats r{};
  std::vector<uint64_t> hi(icore::kBins, 0), lo((size_t)icore::kPercentiles * icore::kBins, 0);
  walk([&](int32_t v, uint32_t key) {
    r.sum_sq += (uint64_t)((int64_t)v * (int64_t)v);
    ++r.count;
    ++hi[key >> 8];
  });
  if (r.count == 0) return r;
  icore::BinRank t[icore::kPercentiles];
  uint32_t slot[icore::kPercentiles];
  for (int j = 0; j < icore::kPercentiles; ++j)
    t[j] = icore::select_bin(hi.data(), icore::kBins, icore::percentile_rank(icore::percentile_of(j), r.count));
  icore::share_slots(t, slot);
  walk([&](int32_t, uint32_t key) {
    const int s = icore::slot_of(t, key >> 8);
    if (s >= 0) ++lo[(size_t)s * icore::kBins + (key & 255u)];
  });
  for (int j = 0; j < icore::kPercentiles; ++j) {
    const icore::BinRank l = icore::select_bin(lo.data() + (size_t)slot[j] * icore::kBins, icore::kBins, t[j].rank);
    r.pct[j] = icore::key_sample((uint16_t)((t[j].bin << 8) | l.bin), type);
  }
  return r;
}

double intensity_std(const IntensityStats& st, int64_t raw_sum) {
  if (st.count == 0) return 0.0;
  // n · Σv² − (Σv)² ≥ 0 exactly; the double formula Σv²/n − mean² cancels for 16-bit data.
  const __int128 num = (__int128)st.count * (__int128)st.sum_sq - (__int128)raw_sum * (__int128)raw_sum;
  return std::sqrt((double)num) / (double)st.count;
}

std::string intensity_keys(const IntensityStats& st, int64_t raw_sum, float slope, float intercept, bool apply_rescale) {
  char buf[256];
  std::string s;
  std::snprintf(buf, sizeof buf, ",\"raw_sum_sq\":%llu", (unsigned long long)st.sum_sq);
  s += buf;
  static const char* const raw_keys[5] = {"raw_p10", "raw_p25", "raw_p50", "raw_p75", "raw_p90"};
  static const char* const keys[5] = {"p10", "p25", "median", "p75", "p90"};
  for (int j = 0; j < 5; ++j) {
    std::snprintf(buf, sizeof buf, ",\"%s\":%d", raw_keys[j], st.pct[j]);
    s += buf;
  }
  const bool any = st.count > 0;
  auto put_d = [&](const char* key, double v) {
    if (any)
      std::snprintf(buf, sizeof buf, ",\"%s\":%.9g", key, v);
    else
      std::snprintf(buf, sizeof buf, ",\"%s\":null", key);
    s += buf;
  };
  double sd = any ? intensity_std(st, raw_sum) : 0.0;
  if (apply_rescale) sd *= std::fabs((double)slope);
  put_d("std", sd);
  double p[5];
  for (int j = 0; j < 5; ++j) {
    p[j] = (double)st.pct[j];
    if (apply_rescale) p[j] = p[j] * (double)slope + (double)intercept;
    put_d(keys[j], p[j]);
  }
  put_d("iqr", std::fabs(p[3] - p[1]));
  return s;
}

namespace {
// `text` ends with "}\n": the keys go before the closing brace.
std::string append_keys(std::string text, const std::string& keys) {
  text.insert(text.size() - 2, keys);
  return text;
}
}  // namespace

std::string to_json(const SliceMeasure& m, const IntensityStats& st, int w, int h, float spacing_x, float spacing_y,
                    float slope, float intercept, bool apply_rescale, int connectivity) {
  return append_keys(to_json(m, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity),
                     intensity_keys(st, m.raw_sum, slope, intercept, apply_rescale));
}

std::string to_json(const SliceMeasure& m, const SliceDiameters& d, const IntensityStats& st, int w, int h, float spacing_x,
                    float spacing_y, float slope, float intercept, bool apply_rescale, int connectivity) {
  return append_keys(to_json(m, d, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity),
                     intensity_keys(st, m.raw_sum, slope, intercept, apply_rescale));
}

std::string volume_to_json(const VolumeMeasure& m, const IntensityStats& st, int w, int h, int d, double spacing_x,
                           double spacing_y, double spacing_z, const std::string& spacing_z_source, float slope,
                           float intercept, bool apply_rescale, int connectivity) {
  return append_keys(volume_to_json(m, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source, slope, intercept,
                                    apply_rescale, connectivity),
                     intensity_keys(st, m.raw_sum, slope, intercept, apply_rescale));
}

std::string volume_to_json(const VolumeMeasure& m, const IntensityStats& st, const VolumeLesion* lesions, int count,
                           int lesions_max, int w, int h, int d, double spacing_x, double spacing_y, double spacing_z,
                           const std::string& spacing_z_source, float slope, float intercept, bool apply_rescale,
                           int connectivity) {
  // The lesion text is the global text, then lesions_max and lesions: the intensity keys go between.
  const std::string head = volume_to_json(m, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source, slope, intercept,
                                          apply_rescale, connectivity);
  std::string text = volume_to_json(m, lesions, count, lesions_max, w, h, d, spacing_x, spacing_y, spacing_z,
                                    spacing_z_source, slope, intercept, apply_rescale, connectivity);
  text.insert(head.size() - 2, intensity_keys(st, m.raw_sum, slope, intercept, apply_rescale));
  return text;
}

}  // namespace measure
}  // namespace nm03
