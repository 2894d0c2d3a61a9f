// Golden model of the grey-level co-occurrence matrix (nm03/texture_core.h, nm03/measure.h TextureGlcm),
// the host emulation of the K12 kernels' per-word pair logic, the features derived from a matrix and
// the sidecar text of a record.
//
// golden::measure_texture is the oracle: a loop over the voxels and over the list of forward directions.
// It shares only stored_sample, sample_key and tcore::level with the kernels. measure::texture_words is
// the opposite: the kernels' walk over u64 words with shifted neighbour masks and directed counts,
// without a GPU. measure::glcm_features is the one place where doubles are made from the integers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "nm03/golden.h"
#include "nm03/intensity_core.h"
#include "nm03/measure.h"
#include "nm03/texture_core.h"
#include "nm03/volume.h"

namespace nm03 {

namespace {
void check_levels(int levels, const char* who) {
  if (levels < tcore::kMinLevels || levels > tcore::kMaxLevels)
    throw std::invalid_argument(std::string(who) + ": texture levels must be 2..64 (got " + std::to_string(levels) + ")");
}
}  // namespace

namespace golden {

namespace {
measure::Glcm cooccurrence(const std::vector<uint8_t>& dilated, const std::vector<uint16_t>& raw, int w, int h, int d,
                           PixelType type, int stored_bits, int levels, bool volume) {
  const size_t n = (size_t)w * h * d;
  if (dilated.size() != n || raw.size() != n) throw std::invalid_argument("measure_texture: mask and samples must have one shape");
  if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("measure_texture: stored bits must be 1..16");
  check_levels(levels, "measure_texture");
  measure::Glcm g;
  g.head.levels = (uint32_t)levels;
  g.c.assign((size_t)levels * levels, 0u);
  auto key_at = [&](size_t i) {
    return (uint32_t)icore::sample_key(stored_sample(raw[i], (uint8_t)type, (uint8_t)stored_bits), (uint8_t)type);
  };
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (size_t i = 0; i < n; ++i)
    if (dilated[i]) {
      const uint32_t k = key_at(i);
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
      ++g.head.samples;
    }
  if (g.head.samples == 0) return g;
  if (volume) measure::check_glcm_exact(g.head.samples);  // the cells below are 32-bit as the kernels' are
  g.head.key_lo = lo;
  g.head.key_hi = hi;
  // The forward directions: dz = 1, or dz = 0 and dy = 1, or dz = dy = 0 and dx = 1.
  struct Dir {
    int dx, dy, dz;
  };
  std::vector<Dir> dirs;
  for (int dz = 0; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx)
        if (dz == 1 || (dz == 0 && dy == 1) || (dz == 0 && dy == 0 && dx == 1)) dirs.push_back({dx, dy, dz});
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t i = ((size_t)z * h + y) * w + x;
        if (!dilated[i]) continue;
        const uint32_t a = tcore::level(key_at(i), lo, hi, (uint32_t)levels);
        for (const Dir& t : dirs) {
          const int x2 = x + t.dx, y2 = y + t.dy, z2 = z + t.dz;
          if (x2 < 0 || x2 >= w || y2 < 0 || y2 >= h || z2 < 0 || z2 >= d) continue;
          const size_t j = ((size_t)z2 * h + y2) * w + x2;
          if (!dilated[j]) continue;
          const uint32_t b = tcore::level(key_at(j), lo, hi, (uint32_t)levels);
          ++g.c[(size_t)a * levels + b];
          ++g.c[(size_t)b * levels + a];
          ++g.head.pairs;
        }
      }
  return g;
}
}  // namespace

measure::Glcm measure_texture(const std::vector<uint8_t>& dilated, const SliceInput& s, int levels) {
  if (s.w <= 0 || s.h <= 0) throw std::invalid_argument("measure_texture: empty slice");
  return cooccurrence(dilated, s.raw, s.w, s.h, 1, s.type, s.stored_bits, levels, false);
}

measure::Glcm measure_texture(const std::vector<uint8_t>& dilated, const VolumeInput& v, int levels) {
  if (v.w <= 0 || v.h <= 0 || v.d <= 0) throw std::invalid_argument("measure_texture: empty volume");
  return cooccurrence(dilated, v.raw, v.w, v.h, v.d, v.type, v.stored_bits, levels, true);
}

std::string measure_volume_json(const VolumeMeasure& m, const IntensityStats* st, const std::vector<VolumeLesion>* lesions,
                                int max_lesions, const measure::Glcm& tx, const VolumeInput& v, bool apply_rescale,
                                int connectivity) {
  return measure::volume_to_json(m, st, lesions ? lesions->data() : nullptr, lesions ? (int)lesions->size() : 0,
                                 lesions ? max_lesions : 0, tx, v.w, v.h, v.d, (double)v.spacing_x, (double)v.spacing_y,
                                 v.spacing_z, v.spacing_z_source, v.slope, v.intercept, apply_rescale, connectivity);
}

}  // namespace golden

namespace measure {

Glcm glcm_from_record(const void* p) {
  Glcm g;
  std::memcpy(&g.head, p, sizeof(TextureGlcm));
  check_levels((int)g.head.levels, "glcm_from_record");
  g.c.resize((size_t)g.head.levels * g.head.levels);
  std::memcpy(g.c.data(), static_cast<const uint8_t*>(p) + sizeof(TextureGlcm), g.c.size() * 4);
  return g;
}

void check_glcm_exact(uint64_t samples) {
  if (!tcore::cells_exact(samples, tcore::kDirections3D))
    throw std::invalid_argument("3D texture: " + std::to_string(samples) + " samples under the mask exceed " +
                                std::to_string(tcore::kMaxExactSamples3D) +
                                ", the most whose 13-direction co-occurrence counts fit the matrix's 32-bit cells");
}

Glcm texture_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d, int wpr,
                   uint8_t type, uint8_t stored_bits, int levels) {
  if (w <= 0 || h <= 0 || d <= 0 || wpr < (w + 63) / 64) throw std::invalid_argument("texture_words: bad shape");
  check_levels(levels, "texture_words");
  const int n = (w + 63) / 64;
  // Word (z, y, k) masked to the width, 0 outside the frame (the kernels' BitVolume::at).
  auto word = [&](int z, int y, int k) -> uint64_t {
    if (z < 0 || z >= d || y < 0 || y >= h || k < 0 || k >= n) return 0ull;
    return dilated[((size_t)z * h + y) * wpr + k] & row_word_mask(k, w);
  };
  auto key_at = [&](int z, int y, int x) {
    const uint16_t bits = raw[(size_t)z * raw_plane_stride + (size_t)y * w + (size_t)x];
    return (uint32_t)icore::sample_key(stored_sample(bits, type, stored_bits), type);
  };
  Glcm g;
  g.head.levels = (uint32_t)levels;
  g.c.assign((size_t)levels * levels, 0u);
  // Walk 1: the range and the count.
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int k = 0; k < n; ++k)
        for (uint64_t t = word(z, y, k); t; t &= t - 1) {
          const uint32_t key = key_at(z, y, (k << 6) + __builtin_ctzll(t));
          lo = key < lo ? key : lo;
          hi = key > hi ? key : hi;
          ++g.head.samples;
        }
  if (g.head.samples == 0) return g;
  check_glcm_exact(g.head.samples);  // the 3D bound: a slice of the engine (at most 4096²) never reaches it
  g.head.key_lo = lo;
  g.head.key_hi = hi;
  // Walk 2: directed counts, word by word, over the five partner rows.
  const tcore::Leveler level(lo, hi, (uint32_t)levels);
  std::vector<uint32_t> dir((size_t)levels * levels, 0u);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int k = 0; k < n; ++k) {
        const uint64_t own = word(z, y, k);
        if (!own) continue;
        for (int r = 0; r < tcore::kPairRows; ++r) {
          const int y2 = y + tcore::pair_row_dy(r), z2 = z + tcore::pair_row_dz(r);
          const uint64_t prev = word(z2, y2, k - 1), cur = word(z2, y2, k), next = word(z2, y2, k + 1);
          for (int dx = tcore::pair_row_first_dx(r); dx <= 1; ++dx)
            for (uint64_t t = own & tcore::neighbour_word(prev, cur, next, dx); t; t &= t - 1) {
              const int x = (k << 6) + __builtin_ctzll(t);
              const uint32_t a = level(key_at(z, y, x));
              const uint32_t b = level(key_at(z2, y2, x + dx));
              ++dir[(size_t)a * levels + b];
              ++g.head.pairs;
            }
        }
      }
  for (int a = 0; a < levels; ++a)
    for (int b = 0; b < levels; ++b) g.c[(size_t)a * levels + b] = dir[(size_t)a * levels + b] + dir[(size_t)b * levels + a];
  return g;
}

GlcmFeatures glcm_features(const uint32_t* c, int levels) {
  check_levels(levels, "glcm_features");
  GlcmFeatures f;
  f.levels = (uint64_t)levels;
  uint64_t total = 0;
  for (int i = 0; i < levels; ++i)
    for (int j = 0; j < levels; ++j) {
      const uint64_t v = c[(size_t)i * levels + j];
      const uint64_t dd = (uint64_t)(i > j ? i - j : j - i);
      total += v;
      f.nonzero += v ? 1u : 0u;
      f.max_count = v > f.max_count ? v : f.max_count;
      f.sum_abs_d += dd * v;
      f.sum_d2 += dd * dd * v;
      f.sum_sq += v * v;
    }
  f.pairs = total / 2;
  if (total == 0) return f;
  f.any = true;
  // p = C / Σ C by division, not by a reciprocal: a matrix of one cell has p = 1 and joint_var = 0 exactly.
  const double sum = (double)total;
  std::vector<double> psum(2 * (size_t)levels + 1, 0.0), pdiff((size_t)levels, 0.0);
  for (int i = 0; i < levels; ++i)
    for (int j = 0; j < levels; ++j) {
      const double p = (double)c[(size_t)i * levels + j] / sum;
      f.joint_avg += (double)(i + 1) * p;
    }
  const double mu = f.joint_avg;
  double cov = 0.0;
  for (int i = 0; i < levels; ++i)
    for (int j = 0; j < levels; ++j) {
      const uint32_t v = c[(size_t)i * levels + j];
      if (!v) continue;
      const double p = (double)v / sum;
      const double di = (double)(i + 1) - mu, dj = (double)(j + 1) - mu, dd = (double)(i > j ? i - j : j - i);
      const double s = di + dj;
      f.joint_max = p > f.joint_max ? p : f.joint_max;
      f.joint_var += di * di * p;
      f.joint_entropy -= p * std::log2(p);
      f.asm_ += p * p;
      f.contrast += dd * dd * p;
      f.dissimilarity += dd * p;
      f.inv_diff += p / (1.0 + dd);
      f.inv_diff_moment += p / (1.0 + dd * dd);
      cov += di * dj * p;
      f.autocorrelation += (double)(i + 1) * (double)(j + 1) * p;
      f.cluster_tendency += s * s * p;
      f.cluster_shade += s * s * s * p;
      f.cluster_prominence += s * s * s * s * p;
      psum[(size_t)(i + j + 2)] += p;
      pdiff[(size_t)(i > j ? i - j : j - i)] += p;
    }
  for (double p : psum)
    if (p > 0.0) f.sum_entropy -= p * std::log2(p);
  for (double p : pdiff)
    if (p > 0.0) f.diff_entropy -= p * std::log2(p);
  f.correlation_defined = f.joint_var > 0.0;
  if (f.correlation_defined) f.correlation = cov / f.joint_var;
  return f;
}

std::string texture_keys(const uint32_t* c, int levels) {
  const GlcmFeatures f = glcm_features(c, levels);
  char buf[128];
  std::string s;
  auto put_u = [&](const char* key, uint64_t v) {
    std::snprintf(buf, sizeof buf, ",\"%s\":%llu", key, (unsigned long long)v);
    s += buf;
  };
  auto put_d = [&](const char* key, double v, bool defined) {
    if (defined)
      std::snprintf(buf, sizeof buf, ",\"%s\":%.9g", key, v);
    else
      std::snprintf(buf, sizeof buf, ",\"%s\":null", key);
    s += buf;
  };
  put_u("glcm_levels", f.levels);
  put_u("glcm_pairs", f.pairs);
  put_u("glcm_nonzero", f.nonzero);
  put_u("glcm_max_count", f.max_count);
  put_u("glcm_sum_abs_d", f.sum_abs_d);
  put_u("glcm_sum_d2", f.sum_d2);
  put_u("glcm_sum_sq", f.sum_sq);
  put_d("glcm_joint_max", f.joint_max, f.any);
  put_d("glcm_joint_avg", f.joint_avg, f.any);
  put_d("glcm_joint_var", f.joint_var, f.any);
  put_d("glcm_joint_entropy", f.joint_entropy, f.any);
  put_d("glcm_asm", f.asm_, f.any);
  put_d("glcm_contrast", f.contrast, f.any);
  put_d("glcm_dissimilarity", f.dissimilarity, f.any);
  put_d("glcm_inv_diff", f.inv_diff, f.any);
  put_d("glcm_inv_diff_moment", f.inv_diff_moment, f.any);
  put_d("glcm_correlation", f.correlation, f.any && f.correlation_defined);
  put_d("glcm_autocorrelation", f.autocorrelation, f.any);
  put_d("glcm_cluster_tendency", f.cluster_tendency, f.any);
  put_d("glcm_cluster_shade", f.cluster_shade, f.any);
  put_d("glcm_cluster_prominence", f.cluster_prominence, f.any);
  put_d("glcm_sum_entropy", f.sum_entropy, f.any);
  put_d("glcm_diff_entropy", f.diff_entropy, f.any);
  return s;
}

std::string insert_global_keys(std::string text, const std::string& keys) {
  const size_t at = text.find(",\"lesions_max\":");
  text.insert(at == std::string::npos ? text.size() - 2 : at, keys);  // the text ends with "}\n"
  return text;
}

std::string to_json(const SliceMeasure& m, const SliceDiameters* d, const IntensityStats* st, const Glcm& tx, int w, int h,
                    float spacing_x, float spacing_y, float slope, float intercept, bool apply_rescale, int connectivity) {
  std::string text =
      d && st ? to_json(m, *d, *st, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity)
      : d     ? to_json(m, *d, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity)
      : st    ? to_json(m, *st, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity)
              : to_json(m, w, h, spacing_x, spacing_y, slope, intercept, apply_rescale, connectivity);
  return insert_global_keys(std::move(text), texture_keys(tx.c.data(), (int)tx.head.levels));
}

std::string volume_to_json(const VolumeMeasure& m, const IntensityStats* st, const VolumeLesion* lesions, int count,
                           int lesions_max, const Glcm& tx, int w, int h, int d, double spacing_x, double spacing_y,
                           double spacing_z, const std::string& spacing_z_source, float slope, float intercept,
                           bool apply_rescale, int connectivity) {
  const bool ls = lesions_max > 0;
  std::string text =
      ls && st ? volume_to_json(m, *st, lesions, count, lesions_max, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source,
                                slope, intercept, apply_rescale, connectivity)
      : ls     ? volume_to_json(m, lesions, count, lesions_max, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source, slope,
                                intercept, apply_rescale, connectivity)
      : st     ? volume_to_json(m, *st, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source, slope, intercept,
                                apply_rescale, connectivity)
               : volume_to_json(m, w, h, d, spacing_x, spacing_y, spacing_z, spacing_z_source, slope, intercept, apply_rescale,
                                connectivity);
  return insert_global_keys(std::move(text), texture_keys(tx.c.data(), (int)tx.head.levels));
}

}  // namespace measure
}  // namespace nm03
