// --measure: the cohort table. After a job's final barrier rank 0 reads the sidecars the ranks wrote
// (<out>/<patient>/<stem>_measure.json, measure::to_json) in patient / slice order and writes
// <out>/measurements.csv. Reading the files — not gathering records over the comm — keeps the
// table identical at any rank count and batch size, and under --resume.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>

#include "nm03/app.h"
#include "nm03/cohort.h"
#include "nm03/measure.h"

namespace nm03::app {

const char* slice_status_name(int code) {
  switch (code) {
    case kSliceOk: return "ok";
    case kSliceLoadError: return "load_error";
    case kSliceTooSmall: return "too_small";
    case kSliceDeviceError: return "device_error";
    case kSliceExportError: return "export_error";
    default: return "not_run";
  }
}

namespace {

// Columns after patient, file, status: the sidecar's keys in its order, bbox flattened.
const char* const kColumns[] = {"width",      "height",        "connectivity",  "area_px",    "region_px",  "bbox_x0",
                                "bbox_y0",    "bbox_x1",       "bbox_y1",       "sum_x",      "sum_y",      "perimeter_edges",
                                "components", "largest_px",    "holes",         "raw_sum",    "raw_min",    "raw_max",
                                "area_mm2",   "centroid_x",    "centroid_y",    "centroid_x_mm", "centroid_y_mm", "mean"};
constexpr size_t kNumColumns = sizeof(kColumns) / sizeof(kColumns[0]);
constexpr size_t kColAreaPx = 3, kColAreaMm2 = 18;
// --measure-diameters: the columns after those — the diameter keys in their order, arrays flattened.
const char* const kDiameterColumns[] = {"lesion_px", "lesion_first_x", "lesion_first_y", "major_px2", "major_xa", "major_ya",
                                        "major_xb",  "major_yb",       "perp_extent",    "perp_xc",   "perp_yc",  "perp_xd",
                                        "perp_yd",   "major_mm",       "perp_mm",        "bidimensional_mm2", "major_angle_deg"};
constexpr size_t kNumDiameterColumns = sizeof(kDiameterColumns) / sizeof(kDiameterColumns[0]);
constexpr size_t kColMajorMm = kNumColumns + 13, kColPerpMm = kNumColumns + 14, kColBidimensional = kNumColumns + 15;

// --measure-intensity: the columns after all of those — the intensity keys in their order.
const char* const kIntensityColumns[] = {"raw_sum_sq", "raw_p10", "raw_p25", "raw_p50", "raw_p75", "raw_p90", "std",
                                         "p10",        "p25",     "median",  "p75",     "p90",     "iqr"};
constexpr size_t kNumIntensityColumns = sizeof(kIntensityColumns) / sizeof(kIntensityColumns[0]);
const char* const kIntensityKey = ",\"raw_sum_sq\":";

// --measure-texture: the columns after all of those — the texture keys in their order.
const char* const kTextureColumns[] = {"glcm_levels",          "glcm_pairs",           "glcm_nonzero",
                                       "glcm_max_count",       "glcm_sum_abs_d",       "glcm_sum_d2",
                                       "glcm_sum_sq",          "glcm_joint_max",       "glcm_joint_avg",
                                       "glcm_joint_var",       "glcm_joint_entropy",   "glcm_asm",
                                       "glcm_contrast",        "glcm_dissimilarity",   "glcm_inv_diff",
                                       "glcm_inv_diff_moment", "glcm_correlation",     "glcm_autocorrelation",
                                       "glcm_cluster_tendency", "glcm_cluster_shade",  "glcm_cluster_prominence",
                                       "glcm_sum_entropy",     "glcm_diff_entropy"};
constexpr size_t kNumTextureColumns = sizeof(kTextureColumns) / sizeof(kTextureColumns[0]);
const char* const kTextureKey = ",\"glcm_levels\":";

// The values of one sidecar line in column order ("" for null). The text is this program's own
// (one flat object, one array of four integers): values are what stands between ':' or ',' and the
// next ',' / ']' / '}'.
bool parse_sidecar(const std::string& text, std::vector<std::string>& out, size_t columns = kNumColumns) {
  out.clear();
  size_t i = text.find('{');
  if (i == std::string::npos) return false;
  ++i;
  while (i < text.size() && text[i] != '}') {
    if (text[i] == ',') ++i;
    if (text[i] != '"') return false;
    const size_t kend = text.find('"', i + 1);
    if (kend == std::string::npos || kend + 1 >= text.size() || text[kend + 1] != ':') return false;
    i = kend + 2;
    if (i < text.size() && text[i] == '[') {
      const size_t aend = text.find(']', i);
      if (aend == std::string::npos) return false;
      std::stringstream ss(text.substr(i + 1, aend - i - 1));
      std::string v;
      while (std::getline(ss, v, ',')) out.push_back(v);
      i = aend + 1;
    } else {
      size_t vend = i;
      while (vend < text.size() && text[vend] != ',' && text[vend] != '}') ++vend;
      const std::string v = text.substr(i, vend - i);
      out.push_back(v == "null" ? std::string() : v);
      i = vend;
    }
  }
  return out.size() == columns;
}

// --measure-volume: the columns after patient, status — the volume sidecar's keys in its order, bbox flattened.
const char* const kVolumeColumns[] = {
    "width",      "height",      "depth",      "connectivity", "volume_vox", "region_vox",  "bbox_x0",       "bbox_y0",
    "bbox_z0",    "bbox_x1",     "bbox_y1",    "bbox_z1",      "sum_x",      "sum_y",       "sum_z",         "faces_x",
    "faces_y",    "faces_z",     "components", "largest_vox",  "cavities",   "euler",       "raw_sum",       "raw_min",
    "raw_max",    "tunnels",     "spacing_x",  "spacing_y",    "spacing_z",  "spacing_z_source", "volume_mm3", "volume_ml",
    "surface_mm2", "centroid_x", "centroid_y", "centroid_z",   "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean"};
constexpr size_t kNumVolumeColumns = sizeof(kVolumeColumns) / sizeof(kVolumeColumns[0]);
constexpr size_t kVolColVox = 4, kVolColMm3 = 30;

// --measure-volume-lesions: the columns after patient, lesion — a lesion object's keys in its order, first and
// bbox flattened.
const char* const kLesionColumns[] = {
    "voxels",     "first_x",    "first_y",   "first_z",       "bbox_x0",       "bbox_y0",       "bbox_z0", "bbox_x1",
    "bbox_y1",    "bbox_z1",    "sum_x",     "sum_y",         "sum_z",         "faces_x",       "faces_y", "faces_z",
    "raw_sum",    "raw_min",    "raw_max",   "volume_mm3",    "volume_ml",     "surface_mm2",   "equivalent_diameter_mm",
    "centroid_x", "centroid_y", "centroid_z", "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean"};
constexpr size_t kNumLesionColumns = sizeof(kLesionColumns) / sizeof(kLesionColumns[0]);
const char* const kLesionsKey = ",\"lesions_max\":";
// --measure-volume-diameters: the columns after those — a lesion object's diameter keys in their order, arrays flattened.
const char* const kLesionDiameterColumns[] = {
    "major_um2",     "major_xa",      "major_ya",         "major_za",      "major_xb",      "major_yb",      "major_zb",
    "axial_z",       "axial_um2",     "axial_xa",         "axial_ya",      "axial_xb",      "axial_yb",      "axial_perp_extent",
    "axial_perp_xc", "axial_perp_yc", "axial_perp_xd",    "axial_perp_yd", "diameter_3d_mm", "axial_major_mm", "axial_perp_mm",
    "axial_bidimensional_mm2"};
constexpr size_t kNumLesionDiameterColumns = sizeof(kLesionDiameterColumns) / sizeof(kLesionDiameterColumns[0]);
constexpr size_t kLesionColDiameter3d = kNumLesionColumns + 18;
const char* const kDiametersSpacingKey = ",\"diameters_spacing_um\":";

// The volume sidecar's text without the lesion keys (and the diameters' spacing key in front of them): what
// --measure-volume alone writes.
std::string without_lesions(const std::string& text) {
  size_t at = text.find(kDiametersSpacingKey);
  if (at == std::string::npos) at = text.find(kLesionsKey);
  return at == std::string::npos ? text : text.substr(0, at) + "}\n";
}

// A sidecar's text without the intensity keys (they are the last keys of a flat object, or stand before
// the lesion keys, which the caller has cut), and those keys' 13 values in `intensity` when there are any.
std::string without_intensity(const std::string& text, std::vector<std::string>* intensity) {
  const size_t at = text.find(kIntensityKey);
  if (at == std::string::npos) return text;
  std::vector<std::string> v;
  if (intensity && parse_sidecar("{" + text.substr(at + 1), v, kNumIntensityColumns)) *intensity = v;
  return text.substr(0, at) + "}\n";
}

// Likewise the texture keys: the last keys of a sidecar whose lesion keys the caller has cut.
std::string without_texture(const std::string& text, std::vector<std::string>* texture) {
  const size_t at = text.find(kTextureKey);
  if (at == std::string::npos) return text;
  std::vector<std::string> v;
  if (texture && parse_sidecar("{" + text.substr(at + 1), v, kNumTextureColumns)) *texture = v;
  return text.substr(0, at) + "}\n";
}

// --measure-volume-thickness: the columns after all of those. The sidecar's thickness keys (the last global
// keys) hold nine values: thickness_spacing_um's three, which have no column, then these six.
const char* const kThicknessColumns[] = {"inscribed_um2", "inscribed_x", "inscribed_y", "inscribed_z", "inscribed_radius_mm",
                                         "thickness_mm"};
constexpr size_t kNumThicknessColumns = sizeof(kThicknessColumns) / sizeof(kThicknessColumns[0]);
constexpr size_t kNumThicknessValues = kNumThicknessColumns + 3;
const char* const kThicknessKey = ",\"thickness_spacing_um\":";

// Likewise the thickness keys: the last keys of a sidecar whose lesion keys the caller has cut.
std::string without_thickness(const std::string& text, std::vector<std::string>* thickness) {
  const size_t at = text.find(kThicknessKey);
  if (at == std::string::npos) return text;
  std::vector<std::string> v;
  if (thickness && parse_sidecar("{" + text.substr(at + 1), v, kNumThicknessValues)) *thickness = v;
  return text.substr(0, at) + "}\n";
}

// The texture columns of one row: the values, or empty fields.
void put_texture(std::ostringstream& o, bool have, const std::vector<std::string>& tv) {
  for (size_t c = 0; c < kNumTextureColumns; ++c) o << "," << (have && tv.size() == kNumTextureColumns ? tv[c] : std::string());
}

// ", \"texture\": true, \"texture_levels\": N" before the closing brace of a --json totals object.
void put_texture_totals(std::string& s, int levels) {
  if (levels) s.insert(s.size() - 1, ", \"texture\": true, \"texture_levels\": " + std::to_string(levels));
}

}  // namespace

VolumeTotals write_volumes_csv(const std::string& out_root, const std::vector<VolumePatientRow>& rows, bool intensity,
                               int texture_levels, bool thickness) {
  VolumeTotals tot;
  tot.intensity = intensity;
  tot.texture_levels = texture_levels;
  tot.thickness = thickness;
  std::ostringstream o;
  o << "patient,status";
  for (const char* c : kVolumeColumns) o << "," << c;
  if (intensity)
    for (const char* c : kIntensityColumns) o << "," << c;
  if (texture_levels)
    for (const char* c : kTextureColumns) o << "," << c;
  if (thickness)
    for (const char* c : kThicknessColumns) o << "," << c;
  o << "\n";
  for (const auto& r : rows) {
    std::vector<std::string> v, iv, tv, hv;
    const bool have =
        r.ok && parse_sidecar(without_intensity(without_texture(without_thickness(without_lesions(r.sidecar), &hv), &tv), &iv), v,
                              kNumVolumeColumns);
    o << r.id << "," << (r.ok ? (have ? "ok" : "no_sidecar") : "failed");
    for (size_t c = 0; c < kNumVolumeColumns; ++c) {
      std::string x = have ? v[c] : std::string();
      if (x.size() >= 2 && x.front() == '"' && x.back() == '"') x = x.substr(1, x.size() - 2);
      o << "," << x;
    }
    if (intensity)
      for (size_t c = 0; c < kNumIntensityColumns; ++c) o << "," << (have && iv.size() == kNumIntensityColumns ? iv[c] : std::string());
    if (texture_levels) put_texture(o, have, tv);
    if (thickness) {
      const bool hh = have && hv.size() == kNumThicknessValues;
      for (size_t c = 0; c < kNumThicknessColumns; ++c) o << "," << (hh ? hv[3 + c] : std::string());
      if (hh) tot.thickness_mm_max = std::max(tot.thickness_mm_max, std::strtod(hv[3 + 5].c_str(), nullptr));
    }
    o << "\n";
    if (!have) continue;
    ++tot.volumes;
    tot.volume_vox += std::strtoull(v[kVolColVox].c_str(), nullptr, 10);
    tot.volume_mm3 += std::strtod(v[kVolColMm3].c_str(), nullptr);
  }
  const std::string text = o.str();
  std::ofstream f(cohort::with_slash(out_root) + "volumes.csv", std::ios::binary | std::ios::trunc);
  f.write(text.data(), (std::streamsize)text.size());
  if (!f) throw std::runtime_error("Cannot write " + cohort::with_slash(out_root) + "volumes.csv");
  return tot;
}

std::string volume_totals_json(const VolumeTotals& t) {
  char buf[240];
  if (t.lesions >= 0)
    std::snprintf(buf, sizeof buf,
                  "{\"volumes\": %lld, \"volume_vox_total\": %llu, \"volume_mm3_total\": %.9g, \"lesions\": %lld}",
                  (long long)t.volumes, (unsigned long long)t.volume_vox, t.volume_mm3, (long long)t.lesions);
  else
    std::snprintf(buf, sizeof buf, "{\"volumes\": %lld, \"volume_vox_total\": %llu, \"volume_mm3_total\": %.9g}",
                  (long long)t.volumes, (unsigned long long)t.volume_vox, t.volume_mm3);
  std::string s = buf;
  if (t.intensity) s.insert(s.size() - 1, ", \"intensity\": true");
  put_texture_totals(s, t.texture_levels);
  if (t.thickness) {
    std::snprintf(buf, sizeof buf, ", \"thickness\": true, \"thickness_mm_max\": %.9g", t.thickness_mm_max);
    s.insert(s.size() - 1, buf);
  }
  if (t.diameters) {
    std::snprintf(buf, sizeof buf, ", \"diameters\": true, \"diameter_3d_mm_max\": %.9g", t.diameter_3d_mm_max);
    s.insert(s.size() - 1, buf);
  }
  return s;
}

int64_t write_lesions_csv(const std::string& out_root, const std::vector<VolumePatientRow>& rows, bool diameters,
                          VolumeTotals* totals) {
  int64_t total = 0;
  double d3max = 0;
  const size_t ncols = kNumLesionColumns + (diameters ? kNumLesionDiameterColumns : 0);
  std::ostringstream o;
  o << "patient,lesion";
  for (const char* c : kLesionColumns) o << "," << c;
  if (diameters)
    for (const char* c : kLesionDiameterColumns) o << "," << c;
  o << "\n";
  auto empty_row = [&](const std::string& id, const char* status) {
    o << id << "," << status;
    for (size_t c = 0; c < ncols; ++c) o << ",";
    o << "\n";
  };
  for (const auto& r : rows) {
    if (!r.ok) {
      empty_row(r.id, "failed");
      continue;
    }
    // The array of flat objects after "lesions":[ — each one parses like a sidecar of its own.
    const size_t key = r.sidecar.find(kLesionsKey);
    const size_t open = key == std::string::npos ? key : r.sidecar.find('[', key);
    if (open == std::string::npos) {
      empty_row(r.id, "no_sidecar");
      continue;
    }
    int rank = 0;
    for (size_t i = r.sidecar.find('{', open); i != std::string::npos; i = r.sidecar.find('{', i)) {
      const size_t end = r.sidecar.find('}', i);
      if (end == std::string::npos) break;
      std::vector<std::string> v;
      // A lesion object has the diameter keys or not, whatever this run asked for (a sidecar of an earlier run).
      const std::string obj = r.sidecar.substr(i, end - i + 1);
      if (!parse_sidecar(obj, v, kNumLesionColumns + kNumLesionDiameterColumns) && !parse_sidecar(obj, v, kNumLesionColumns)) break;
      if (diameters && v.size() == ncols && !v[kLesionColDiameter3d].empty())
        d3max = std::max(d3max, std::strtod(v[kLesionColDiameter3d].c_str(), nullptr));
      v.resize(ncols);
      o << r.id << "," << rank++;
      for (const auto& x : v) o << "," << x;
      o << "\n";
      ++total;
      i = end;
    }
  }
  const std::string text = o.str();
  std::ofstream f(cohort::with_slash(out_root) + "lesions.csv", std::ios::binary | std::ios::trunc);
  f.write(text.data(), (std::streamsize)text.size());
  if (!f) throw std::runtime_error("Cannot write " + cohort::with_slash(out_root) + "lesions.csv");
  if (totals) totals->diameters = diameters, totals->diameter_3d_mm_max = d3max;
  return total;
}

MeasureTotals write_measurements_csv(const std::string& out_root, const std::vector<MeasurePatient>& patients,
                                     bool diameters, bool intensity, int texture_levels) {
  MeasureTotals tot;
  tot.diameters = diameters;
  tot.intensity = intensity;
  tot.texture_levels = texture_levels;
  const size_t ncols = kNumColumns + (diameters ? kNumDiameterColumns : 0);
  std::ostringstream o;
  o << "patient,file,status";
  for (const char* c : kColumns) o << "," << c;
  if (diameters)
    for (const char* c : kDiameterColumns) o << "," << c;
  if (intensity)
    for (const char* c : kIntensityColumns) o << "," << c;
  if (texture_levels)
    for (const char* c : kTextureColumns) o << "," << c;
  o << "\n";
  char buf[64];
  for (const auto& p : patients) {
    uint64_t area_px = 0;
    double area_mm2 = 0;
    // The patient's slice of the largest bidimensional_mm2 (the first one of that value).
    bool have_bidim = false;
    double bidim = 0;
    std::string bidim_text, major_text, perp_text;
    for (size_t i = 0; i < p.files.size(); ++i) {
      const std::string name = cohort::filename(p.files[i]);
      std::vector<std::string> v, iv, tv;
      bool have = false;
      if (p.status[i] == kSliceOk) {
        std::ifstream f(cohort::with_slash(p.out_dir) + measure::sidecar_name(cohort::stem(p.files[i])), std::ios::binary);
        std::stringstream ss;
        if (f) ss << f.rdbuf();
        // With `diameters` a sidecar without the diameter keys (written earlier without the flag) is read too.
        // With `intensity` the intensity keys, the sidecar's last, go to their own columns; without them
        // (a sidecar written earlier without the flag) those columns stay empty.
        // The texture keys come after them and are cut first, whether the table has their columns or not.
        const std::string cut = without_texture(ss.str(), &tv);
        const std::string text = intensity ? without_intensity(cut, &iv) : cut;
        have = f && (parse_sidecar(text, v, ncols) || (diameters && parse_sidecar(text, v, kNumColumns)));
        if (have) v.resize(ncols);
      }
      o << p.id << "," << name << "," << (p.status[i] == kSliceOk && !have ? "no_sidecar" : slice_status_name(p.status[i]));
      for (size_t c = 0; c < ncols; ++c) o << "," << (have ? v[c] : std::string());
      if (intensity)
        for (size_t c = 0; c < kNumIntensityColumns; ++c) o << "," << (have && iv.size() == kNumIntensityColumns ? iv[c] : std::string());
      if (texture_levels) put_texture(o, have, tv);
      o << "\n";
      if (!have) continue;
      ++tot.slices;
      area_px += std::strtoull(v[kColAreaPx].c_str(), nullptr, 10);
      area_mm2 += std::strtod(v[kColAreaMm2].c_str(), nullptr);
      if (diameters && !v[kColBidimensional].empty()) {
        const double b = std::strtod(v[kColBidimensional].c_str(), nullptr);
        if (!have_bidim || b > bidim)
          have_bidim = true, bidim = b, bidim_text = v[kColBidimensional], major_text = v[kColMajorMm], perp_text = v[kColPerpMm];
      }
    }
    o << p.id << ",TOTAL,";
    for (size_t c = 0; c < ncols; ++c) {
      o << ",";
      if (c == kColAreaPx) o << area_px;
      if (c == kColAreaMm2) {
        std::snprintf(buf, sizeof buf, "%.9g", area_mm2);
        o << buf;
      }
      if (diameters && c == kColMajorMm) o << major_text;
      if (diameters && c == kColPerpMm) o << perp_text;
      if (diameters && c == kColBidimensional) o << bidim_text;
    }
    if (intensity)
      for (size_t c = 0; c < kNumIntensityColumns; ++c) o << ",";
    if (texture_levels) put_texture(o, false, {});
    o << "\n";
    tot.area_px += area_px;
    tot.area_mm2 += area_mm2;
    if (have_bidim && bidim > tot.bidimensional_mm2_max) tot.bidimensional_mm2_max = bidim;
  }
  const std::string text = o.str();
  std::ofstream f(cohort::with_slash(out_root) + "measurements.csv", std::ios::binary | std::ios::trunc);
  f.write(text.data(), (std::streamsize)text.size());
  if (!f) throw std::runtime_error("Cannot write " + cohort::with_slash(out_root) + "measurements.csv");
  return tot;
}

std::string measure_totals_json(const MeasureTotals& t) {
  char buf[240];
  if (t.diameters)
    std::snprintf(buf, sizeof buf,
                  "{\"slices\": %lld, \"area_px_total\": %llu, \"area_mm2_total\": %.9g, \"bidimensional_mm2_max\": %.9g}",
                  (long long)t.slices, (unsigned long long)t.area_px, t.area_mm2, t.bidimensional_mm2_max);
  else
    std::snprintf(buf, sizeof buf, "{\"slices\": %lld, \"area_px_total\": %llu, \"area_mm2_total\": %.9g}", (long long)t.slices,
                  (unsigned long long)t.area_px, t.area_mm2);
  std::string s = buf;
  if (t.intensity) s.insert(s.size() - 1, ", \"intensity\": true");
  put_texture_totals(s, t.texture_levels);
  return s;
}

}  // namespace nm03::app
