// pybind11 module `_nm03` — Python surface of the native engine (package nm03_capstone_project_amd).
// Host codecs, golden model, engine, 3D mode, comm self-tests, and raw-pointer kernel entry points
// that the torch-tensor wrappers in nm03_capstone_project_amd/ops use (device pointers + stream).
#include <hip/hip_runtime_api.h>
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sys/mman.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "nm03/app.h"
#include "nm03/cohort.h"
#include "nm03/comm.h"
#include "nm03/cpu_sampler.h"
#include "nm03/dicom.h"
#include "nm03/engine.h"
#include "nm03/metaimage.h"
#include "nm03/numa.h"
#include "nm03/golden.h"
#include "nm03/intensity_core.h"
#include "nm03/jpeg.h"
#include "nm03/jpeg_dct.h"
#include "nm03/jpeg_lossless.h"
#include "nm03/kernels.h"
#include "nm03/synth.h"
#include "nm03/texture_core.h"
#include "nm03/volume.h"
#include "nm03/volume_compare.h"
#include "nm03/volume_compare_core.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_slabs.h"

namespace py = pybind11;
using namespace nm03;

namespace {

template <class T>
py::array_t<T> to_np(const std::vector<T>& v, std::vector<py::ssize_t> shape) {
  py::array_t<T> a(shape);
  std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

template <class T>
std::vector<T> from_np(const py::array_t<T, py::array::c_style | py::array::forcecast>& a) {
  return std::vector<T>(a.data(), a.data() + a.size());
}

PixelType parse_type(const std::string& t) {
  if (t == "u16") return kU16;
  if (t == "i16") return kI16;
  if (t == "u8") return kU8;
  throw std::invalid_argument("pixel type must be u16, i16 or u8");
}

golden::SliceInput slice_from(py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                              int stored_bits, float slope, float intercept, float sx, float sy) {
  if (raw.ndim() != 2) throw std::invalid_argument("raw must be a 2D uint16 array");
  golden::SliceInput s;
  s.h = (int)raw.shape(0);
  s.w = (int)raw.shape(1);
  s.type = parse_type(type);
  if (s.type == kU8) s.type = kU16;
  s.stored_bits = stored_bits;
  s.slope = slope;
  s.intercept = intercept;
  s.spacing_x = sx;
  s.spacing_y = sy;
  s.raw = from_np<uint16_t>(raw);
  return s;
}

py::dict header_dict(const dicom::Header& h) {
  py::dict d;
  d["rows"] = h.rows;
  d["cols"] = h.cols;
  d["bits_allocated"] = h.bits_allocated;
  d["bits_stored"] = h.bits_stored;
  d["pixel_representation"] = h.pixel_rep;
  d["type"] = h.type == kU16 ? "u16" : h.type == kI16 ? "i16" : "u8";
  d["has_rescale"] = h.has_rescale;
  d["slope"] = h.slope;
  d["intercept"] = h.intercept;
  d["spacing_x"] = h.spacing_x;
  d["spacing_y"] = h.spacing_y;
  d["instance_number"] = h.instance_number;
  d["transfer_syntax"] = h.transfer_syntax;
  d["photometric"] = h.photometric;
  d["patient_id"] = h.patient_id;
  d["modality"] = h.modality;
  d["sop_instance_uid"] = h.sop_instance_uid;
  d["series_uid"] = h.series_uid;
  d["pixel_offset"] = h.pixel_offset;
  d["pixel_length"] = h.pixel_length;
  d["frames"] = h.frames;
  d["invert"] = h.invert;
  d["syntax"] = dicom::syntax_name(h.syntax);
  return d;
}

std::vector<Seed> seeds_from(const std::vector<std::tuple<int, int, int>>& s) {
  std::vector<Seed> v;
  for (auto& t : s) v.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t)});
  return v;
}

py::array_t<uint8_t> mask2d(const std::vector<uint8_t>& v, int h, int w) { return to_np<uint8_t>(v, {h, w}); }

// ---- device scratch for the raw-pointer kernel entry points --------------------------------
struct Scratch {
  void* p = nullptr;
  size_t cap = 0;
  void* get(size_t bytes) {
    if (bytes > cap) {
      if (p) (void)hipFree(p);
      cap = std::max<size_t>(bytes, 1 << 20);
      gpu::check_hip(hipMalloc(&p, cap), "hipMalloc scratch");
    }
    return p;
  }
};
Scratch& scratch() {
  static Scratch s;
  return s;
}

hipStream_t as_stream(uintptr_t s) { return reinterpret_cast<hipStream_t>(s); }

// Builds SliceDesc/TileDesc tables for n equally sized slices laid out contiguously
// (raw/med: n×h×w u16; masks: n×h×wpr words) and uploads them (synchronously) to scratch.
struct BatchTables {
  gpu::SliceDesc* desc;
  gpu::TileDesc* medt;
  gpu::TileDesc* shpt;
  gpu::SeedXY* seeds;
  gpu::SliceStats* stats;
  int nmed, nshp;
};

BatchTables upload_tables(int n, int h, int w, PixelType type, int stored_bits, float slope, float intercept,
                          const std::vector<Seed>& seeds, hipStream_t st) {
  std::vector<gpu::SliceDesc> d(n);
  std::vector<gpu::TileDesc> mt, sh;
  std::vector<gpu::SeedXY> sd;
  const int wpr = (w + 63) / 64;
  for (int i = 0; i < n; ++i) {
    gpu::SliceDesc& s = d[i];
    std::memset(&s, 0, sizeof(s));
    s.raw_off = (uint32_t)((size_t)i * h * w);
    s.mask_off = (uint32_t)((size_t)i * h * wpr);
    s.f32_off = s.raw_off;
    s.w = (uint16_t)w;
    s.h = (uint16_t)h;
    s.wpr = (uint16_t)wpr;
    s.type = type == kU8 ? kU16 : type;
    s.stored_bits = (uint8_t)stored_bits;
    s.slope = slope;
    s.intercept = intercept;
    s.seed_off = (uint32_t)sd.size();
    s.seed_count = (uint16_t)seeds.size();
    for (auto& q : seeds) sd.push_back({(int16_t)q.x, (int16_t)q.y});
    for (int ty = 0; ty < (h + 63) / 64; ++ty)
      for (int tx = 0; tx < (w + 63) / 64; ++tx) mt.push_back({(uint32_t)i, (uint16_t)tx, (uint16_t)ty});
    for (int ty = 0; ty < (h + gpu::kShpTileH - 1) / gpu::kShpTileH; ++ty)
      for (int tx = 0; tx < wpr; ++tx) sh.push_back({(uint32_t)i, (uint16_t)tx, (uint16_t)ty});
  }
  if (sd.empty()) sd.push_back({0, 0});
  std::vector<gpu::SliceStats> stats(n, gpu::SliceStats{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u});
  const size_t o1 = 0, o2 = o1 + d.size() * sizeof(gpu::SliceDesc), o3 = (o2 + mt.size() * 8 + 255) / 256 * 256,
               o4 = (o3 + sh.size() * 8 + 255) / 256 * 256, o5 = (o4 + sd.size() * 4 + 255) / 256 * 256,
               total = o5 + stats.size() * sizeof(gpu::SliceStats);
  std::vector<uint8_t> blob(total);
  std::memcpy(blob.data() + o1, d.data(), d.size() * sizeof(gpu::SliceDesc));
  std::memcpy(blob.data() + o2, mt.data(), mt.size() * 8);
  std::memcpy(blob.data() + o3, sh.data(), sh.size() * 8);
  std::memcpy(blob.data() + o4, sd.data(), sd.size() * 4);
  std::memcpy(blob.data() + o5, stats.data(), stats.size() * sizeof(gpu::SliceStats));
  uint8_t* dev = (uint8_t*)scratch().get(total);
  gpu::check_hip(hipMemcpyAsync(dev, blob.data(), total, hipMemcpyHostToDevice, st), "H2D tables");
  gpu::check_hip(hipStreamSynchronize(st), "sync tables");
  return BatchTables{(gpu::SliceDesc*)(dev + o1), (gpu::TileDesc*)(dev + o2), (gpu::TileDesc*)(dev + o3),
                     (gpu::SeedXY*)(dev + o4), (gpu::SliceStats*)(dev + o5), (int)mt.size(), (int)sh.size()};
}

gpu::PipeConsts consts_from(const PipelineParams& p, int border_radius) {
  gpu::PipeConsts pc{};
  pc.nmin = p.norm_min;
  pc.nmax = p.norm_max;
  pc.nlow = p.norm_low;
  pc.nhigh = p.norm_high;
  pc.cmin = p.clip_min;
  pc.cmax = p.clip_max;
  pc.gain = p.sharpen_gain;
  pc.band_lo = p.srg_min;
  pc.band_hi = p.srg_max;
  gaussian_taps(p.sharpen_sigma, p.sharpen_mask, pc.taps);
  pc.mask_radius = p.sharpen_mask / 2;
  pc.median_k = p.median_window;
  pc.connectivity = p.srg_connectivity == 8 ? 8 : 4;
  pc.dilation_size = p.dilation_size;
  pc.erosion_size = p.erosion_size;
  pc.border_radius = border_radius;
  pc.se_disc = p.se_shape == kSeDisc ? 1 : 0;
  return pc;
}

// The integers of a measurement record (nm03/measure.h) as a dict.
py::dict measure_dict(const SliceMeasure& m) {
  py::dict d;
  d["area_px"] = m.area_px;
  d["region_px"] = m.region_px;
  py::list bb;
  for (int k = 0; k < 4; ++k) bb.append(m.bbox[k]);
  d["bbox"] = bb;
  d["sum_x"] = m.sum_x;
  d["sum_y"] = m.sum_y;
  d["perimeter_edges"] = m.perimeter_edges;
  d["components"] = m.components;
  d["largest_px"] = m.largest_px;
  d["holes"] = m.holes;
  d["raw_sum"] = m.raw_sum;
  d["raw_min"] = m.raw_min;
  d["raw_max"] = m.raw_max;
  return d;
}

SliceMeasure measure_from(const py::dict& d) {
  SliceMeasure m{};
  m.area_px = d["area_px"].cast<uint32_t>();
  m.region_px = d["region_px"].cast<uint32_t>();
  const std::vector<int> bb = d["bbox"].cast<std::vector<int>>();
  if (bb.size() != 4) throw std::invalid_argument("bbox must have four values");
  for (int k = 0; k < 4; ++k) m.bbox[k] = bb[(size_t)k];
  m.sum_x = d["sum_x"].cast<uint64_t>();
  m.sum_y = d["sum_y"].cast<uint64_t>();
  m.perimeter_edges = d["perimeter_edges"].cast<uint32_t>();
  m.components = d["components"].cast<uint32_t>();
  m.largest_px = d["largest_px"].cast<uint32_t>();
  m.holes = d["holes"].cast<uint32_t>();
  m.raw_sum = d["raw_sum"].cast<int64_t>();
  m.raw_min = d["raw_min"].cast<int32_t>();
  m.raw_max = d["raw_max"].cast<int32_t>();
  return m;
}

// The integers of a diameter record (nm03/measure.h SliceDiameters) as a dict.
py::dict diameters_dict(const SliceDiameters& m) {
  py::dict d;
  d["lesion_px"] = m.lesion_px;
  d["lesion_first"] = py::make_tuple(m.lesion_first[0], m.lesion_first[1]).cast<py::list>();
  d["major_px2"] = m.major_px2;
  py::list a, b;
  for (int k = 0; k < 4; ++k) a.append(m.major[k]), b.append(m.perp[k]);
  d["major"] = a;
  d["perp_extent"] = m.perp_extent;
  d["perp"] = b;
  return d;
}

SliceDiameters diameters_from(const py::dict& d) {
  SliceDiameters m{};
  m.lesion_px = d["lesion_px"].cast<uint32_t>();
  const std::vector<int> f = d["lesion_first"].cast<std::vector<int>>(), a = d["major"].cast<std::vector<int>>(),
                         b = d["perp"].cast<std::vector<int>>();
  if (f.size() != 2 || a.size() != 4 || b.size() != 4) throw std::invalid_argument("lesion_first needs two values, major and perp four");
  m.lesion_first[0] = f[0], m.lesion_first[1] = f[1];
  m.major_px2 = d["major_px2"].cast<uint32_t>();
  m.perp_extent = d["perp_extent"].cast<uint32_t>();
  for (int k = 0; k < 4; ++k) m.major[k] = a[(size_t)k], m.perp[k] = b[(size_t)k];
  return m;
}

// The integers of an intensity record (nm03/measure.h IntensityStats) as a dict.
py::dict intensity_dict(const IntensityStats& s) {
  py::dict d;
  d["count"] = s.count;
  d["raw_sum_sq"] = s.sum_sq;
  d["raw_p10"] = s.pct[0];
  d["raw_p25"] = s.pct[1];
  d["raw_p50"] = s.pct[2];
  d["raw_p75"] = s.pct[3];
  d["raw_p90"] = s.pct[4];
  return d;
}

IntensityStats intensity_from(const py::dict& d) {
  IntensityStats s{};
  s.count = d["count"].cast<uint64_t>();
  s.sum_sq = d["raw_sum_sq"].cast<uint64_t>();
  static const char* const keys[5] = {"raw_p10", "raw_p25", "raw_p50", "raw_p75", "raw_p90"};
  for (int j = 0; j < 5; ++j) s.pct[j] = d[keys[j]].cast<int32_t>();
  return s;
}

// A texture record (nm03/measure.h TextureGlcm and its matrix) as a dict: the header integers plus
// `glcm`, the [levels, levels] uint32 matrix.
py::dict texture_dict(const measure::Glcm& g) {
  py::dict d;
  d["levels"] = g.head.levels;
  d["key_lo"] = g.head.key_lo;
  d["key_hi"] = g.head.key_hi;
  d["samples"] = g.head.samples;
  d["pairs"] = g.head.pairs;
  py::array_t<uint32_t> a({(py::ssize_t)g.head.levels, (py::ssize_t)g.head.levels});
  std::memcpy(a.mutable_data(), g.c.data(), g.c.size() * 4);
  d["glcm"] = a;
  return d;
}

measure::Glcm texture_from(const py::dict& d) {
  measure::Glcm g;
  g.head.levels = d["levels"].cast<uint32_t>();
  g.head.key_lo = d["key_lo"].cast<uint32_t>();
  g.head.key_hi = d["key_hi"].cast<uint32_t>();
  g.head.samples = d["samples"].cast<uint64_t>();
  g.head.pairs = d["pairs"].cast<uint64_t>();
  auto a = d["glcm"].cast<py::array_t<uint32_t, py::array::c_style | py::array::forcecast>>();
  if (g.head.levels < 2 || g.head.levels > 64 || a.ndim() != 2 || a.shape(0) != (py::ssize_t)g.head.levels ||
      a.shape(1) != (py::ssize_t)g.head.levels)
    throw std::invalid_argument("texture: glcm must be [levels, levels] with 2 <= levels <= 64");
  g.c.assign(a.data(), a.data() + a.size());
  return g;
}

py::dict glcm_features_dict(const measure::GlcmFeatures& f) {
  py::dict d;
  d["glcm_levels"] = f.levels;
  d["glcm_pairs"] = f.pairs;
  d["glcm_nonzero"] = f.nonzero;
  d["glcm_max_count"] = f.max_count;
  d["glcm_sum_abs_d"] = f.sum_abs_d;
  d["glcm_sum_d2"] = f.sum_d2;
  d["glcm_sum_sq"] = f.sum_sq;
  auto put = [&](const char* k, double v, bool defined) { d[k] = defined ? py::object(py::float_(v)) : py::object(py::none()); };
  put("glcm_joint_max", f.joint_max, f.any);
  put("glcm_joint_avg", f.joint_avg, f.any);
  put("glcm_joint_var", f.joint_var, f.any);
  put("glcm_joint_entropy", f.joint_entropy, f.any);
  put("glcm_asm", f.asm_, f.any);
  put("glcm_contrast", f.contrast, f.any);
  put("glcm_dissimilarity", f.dissimilarity, f.any);
  put("glcm_inv_diff", f.inv_diff, f.any);
  put("glcm_inv_diff_moment", f.inv_diff_moment, f.any);
  put("glcm_correlation", f.correlation, f.any && f.correlation_defined);
  put("glcm_autocorrelation", f.autocorrelation, f.any);
  put("glcm_cluster_tendency", f.cluster_tendency, f.any);
  put("glcm_cluster_shade", f.cluster_shade, f.any);
  put("glcm_cluster_prominence", f.cluster_prominence, f.any);
  put("glcm_sum_entropy", f.sum_entropy, f.any);
  put("glcm_diff_entropy", f.diff_entropy, f.any);
  return d;
}

// The integers of a volume record (nm03/measure.h VolumeMeasure) as a dict.
py::dict volume_measure_dict(const VolumeMeasure& m) {
  py::dict d;
  d["volume_vox"] = m.volume_vox;
  d["region_vox"] = m.region_vox;
  py::list bb;
  for (int k = 0; k < 6; ++k) bb.append(m.bbox[k]);
  d["bbox"] = bb;
  d["sum_x"] = m.sum_x;
  d["sum_y"] = m.sum_y;
  d["sum_z"] = m.sum_z;
  d["faces_x"] = m.faces_x;
  d["faces_y"] = m.faces_y;
  d["faces_z"] = m.faces_z;
  d["components"] = m.components;
  d["largest_vox"] = m.largest_vox;
  d["cavities"] = m.cavities;
  d["euler"] = m.euler;
  d["raw_sum"] = m.raw_sum;
  d["raw_min"] = m.raw_min;
  d["raw_max"] = m.raw_max;
  return d;
}

VolumeMeasure volume_measure_from(const py::dict& d) {
  VolumeMeasure m{};
  m.volume_vox = d["volume_vox"].cast<uint64_t>();
  m.region_vox = d["region_vox"].cast<uint64_t>();
  const std::vector<int> bb = d["bbox"].cast<std::vector<int>>();
  if (bb.size() != 6) throw std::invalid_argument("bbox must have six values");
  for (int k = 0; k < 6; ++k) m.bbox[k] = bb[(size_t)k];
  m.sum_x = d["sum_x"].cast<uint64_t>();
  m.sum_y = d["sum_y"].cast<uint64_t>();
  m.sum_z = d["sum_z"].cast<uint64_t>();
  m.faces_x = d["faces_x"].cast<uint64_t>();
  m.faces_y = d["faces_y"].cast<uint64_t>();
  m.faces_z = d["faces_z"].cast<uint64_t>();
  m.components = d["components"].cast<uint32_t>();
  m.largest_vox = d["largest_vox"].cast<uint64_t>();
  m.cavities = d["cavities"].cast<uint32_t>();
  m.euler = d["euler"].cast<int64_t>();
  m.raw_sum = d["raw_sum"].cast<int64_t>();
  m.raw_min = d["raw_min"].cast<int32_t>();
  m.raw_max = d["raw_max"].cast<int32_t>();
  return m;
}

// The integers of a lesion record (nm03/measure.h VolumeLesion) as a dict.
py::dict volume_lesion_dict(const VolumeLesion& l) {
  py::dict d;
  d["voxels"] = l.voxels;
  py::list fi, bb;
  for (int k = 0; k < 3; ++k) fi.append(l.first[k]);
  for (int k = 0; k < 6; ++k) bb.append(l.bbox[k]);
  d["first"] = fi;
  d["bbox"] = bb;
  d["sum_x"] = l.sum_x;
  d["sum_y"] = l.sum_y;
  d["sum_z"] = l.sum_z;
  d["faces_x"] = l.faces_x;
  d["faces_y"] = l.faces_y;
  d["faces_z"] = l.faces_z;
  d["raw_sum"] = l.raw_sum;
  d["raw_min"] = l.raw_min;
  d["raw_max"] = l.raw_max;
  return d;
}

py::list volume_lesion_list(const VolumeLesion* l, size_t n) {
  py::list out;
  for (size_t i = 0; i < n; ++i) out.append(volume_lesion_dict(l[i]));
  return out;
}

VolumeLesion volume_lesion_from(const py::dict& d) {
  VolumeLesion l{};
  l.voxels = d["voxels"].cast<uint64_t>();
  const std::vector<int> fi = d["first"].cast<std::vector<int>>(), bb = d["bbox"].cast<std::vector<int>>();
  if (fi.size() != 3 || bb.size() != 6) throw std::invalid_argument("first must have three values, bbox six");
  for (int k = 0; k < 3; ++k) l.first[k] = fi[(size_t)k];
  for (int k = 0; k < 6; ++k) l.bbox[k] = bb[(size_t)k];
  l.sum_x = d["sum_x"].cast<uint64_t>();
  l.sum_y = d["sum_y"].cast<uint64_t>();
  l.sum_z = d["sum_z"].cast<uint64_t>();
  l.faces_x = d["faces_x"].cast<uint64_t>();
  l.faces_y = d["faces_y"].cast<uint64_t>();
  l.faces_z = d["faces_z"].cast<uint64_t>();
  l.raw_sum = d["raw_sum"].cast<int64_t>();
  l.raw_min = d["raw_min"].cast<int32_t>();
  l.raw_max = d["raw_max"].cast<int32_t>();
  return l;
}

// The integers of a lesion's diameter record (nm03/measure.h VolumeLesionDiameters) as a dict.
py::dict volume_diameters_dict(const VolumeLesionDiameters& r) {
  py::dict d;
  d["major_um2"] = r.major_um2;
  py::list mj, ax, pp;
  for (int k = 0; k < 6; ++k) mj.append(r.major[k]);
  for (int k = 0; k < 4; ++k) ax.append(r.axial[k]), pp.append(r.axial_perp[k]);
  d["major"] = mj;
  d["axial_z"] = r.axial_z;
  d["axial_um2"] = r.axial_um2;
  d["axial"] = ax;
  d["axial_perp_extent"] = r.axial_perp_extent;
  d["axial_perp"] = pp;
  return d;
}

VolumeLesionDiameters volume_diameters_from(const py::dict& d) {
  VolumeLesionDiameters r{};
  r.major_um2 = d["major_um2"].cast<uint64_t>();
  r.axial_um2 = d["axial_um2"].cast<uint64_t>();
  r.axial_perp_extent = d["axial_perp_extent"].cast<int64_t>();
  r.axial_z = d["axial_z"].cast<int32_t>();
  const std::vector<int> mj = d["major"].cast<std::vector<int>>(), ax = d["axial"].cast<std::vector<int>>(),
                         pp = d["axial_perp"].cast<std::vector<int>>();
  if (mj.size() != 6 || ax.size() != 4 || pp.size() != 4)
    throw std::invalid_argument("major must have six values, axial and axial_perp four");
  for (int k = 0; k < 6; ++k) r.major[k] = mj[(size_t)k];
  for (int k = 0; k < 4; ++k) r.axial[k] = ax[(size_t)k], r.axial_perp[k] = pp[(size_t)k];
  return r;
}

py::list volume_diameters_list(const VolumeLesionDiameters* r, size_t n) {
  py::list out;
  for (size_t i = 0; i < n; ++i) out.append(volume_diameters_dict(r[i]));
  return out;
}

// (ux, uy, uz) in integer micrometres, each 1 … 2^32 − 1.
void spacing_um_from(const std::vector<int64_t>& v, uint32_t um[3]) {
  if (v.size() != 3) throw std::invalid_argument("spacing_um must be (ux, uy, uz)");
  for (int a = 0; a < 3; ++a) {
    if (v[(size_t)a] < 1 || v[(size_t)a] > 0xFFFFFFFFll) throw std::invalid_argument("spacing_um: every value must be 1 .. 2^32 - 1");
    um[a] = (uint32_t)v[(size_t)a];
  }
}

py::dict volume_thickness_dict(const VolumeThickness& t) {
  py::dict d;
  d["inscribed_um2"] = t.inscribed_um2;
  py::list at;
  for (int k = 0; k < 3; ++k) at.append(t.at[k]);
  d["inscribed_at"] = at;
  d["found"] = t.found != 0;
  if (t.found) {
    const double r = measure::inscribed_radius_mm(t);
    d["inscribed_radius_mm"] = r;
    d["thickness_mm"] = 2.0 * r;
  } else {
    d["inscribed_radius_mm"] = py::none();
    d["thickness_mm"] = py::none();
  }
  return d;
}

VolumeThickness volume_thickness_from(const py::dict& d) {
  VolumeThickness t{};
  t.inscribed_um2 = d["inscribed_um2"].cast<uint64_t>();
  const std::vector<int> at = d["inscribed_at"].cast<std::vector<int>>();
  if (at.size() != 3) throw std::invalid_argument("inscribed_at must be [x, y, z]");
  for (int k = 0; k < 3; ++k) t.at[k] = at[(size_t)k];
  t.found = d["found"].cast<bool>() ? 1 : 0;
  return t;
}

// (ux, uy, uz), the mask's shape and the cap of the distance bindings, checked as the ops check them.
void distance_args(const py::array& mask, const std::vector<int64_t>& spacing_um, uint32_t um[3]) {
  if (mask.ndim() != 3) throw std::invalid_argument("mask must be [D, H, W]");
  if (mask.shape(0) < 1 || mask.shape(1) < 1 || mask.shape(2) < 1) throw std::invalid_argument("empty volume");
  spacing_um_from(spacing_um, um);
}

// The integers of a comparison record (nm03/volume_compare.h VolumeCompare) as a dict, keyed as compare.json.
py::dict volume_compare_dict(const VolumeCompare& c) {
  py::dict d;
  d["a_vox"] = c.a_vox, d["b_vox"] = c.b_vox, d["tp_vox"] = c.tp_vox, d["fp_vox"] = c.fp_vox, d["fn_vox"] = c.fn_vox;
  d["surface_a"] = c.surface_a, d["surface_b"] = c.surface_b;
  const VolumeCompareDirected* dirs[2] = {&c.ab, &c.ba};
  const char* tag[2] = {"_ab", "_ba"};
  for (int i = 0; i < 2; ++i) {
    const VolumeCompareDirected& r = *dirs[i];
    const std::string t = tag[i];
    py::list at;
    for (int k = 0; k < 3; ++k) at.append(r.worst[k]);
    d[py::str("n" + t)] = r.n;
    d[py::str("max_um2" + t)] = r.max_um2;
    d[py::str("worst" + t)] = at;
    d[py::str("sum_um" + t)] = r.sum_um;
    d[py::str("p95_um" + t)] = r.p95_um;
    d[py::str("found" + t)] = r.found != 0;
  }
  return d;
}

VolumeCompare volume_compare_from(const py::dict& d) {
  VolumeCompare c{};
  c.a_vox = d["a_vox"].cast<uint64_t>(), c.b_vox = d["b_vox"].cast<uint64_t>(), c.tp_vox = d["tp_vox"].cast<uint64_t>();
  c.fp_vox = d["fp_vox"].cast<uint64_t>(), c.fn_vox = d["fn_vox"].cast<uint64_t>();
  c.surface_a = d["surface_a"].cast<uint64_t>(), c.surface_b = d["surface_b"].cast<uint64_t>();
  VolumeCompareDirected* dirs[2] = {&c.ab, &c.ba};
  const char* tag[2] = {"_ab", "_ba"};
  for (int i = 0; i < 2; ++i) {
    VolumeCompareDirected& r = *dirs[i];
    const std::string t = tag[i];
    r.n = d[py::str("n" + t)].cast<uint32_t>();
    r.max_um2 = d[py::str("max_um2" + t)].cast<uint64_t>();
    const std::vector<int> at = d[py::str("worst" + t)].cast<std::vector<int>>();
    if (at.size() != 3) throw std::invalid_argument("worst must be [x, y, z]");
    for (int k = 0; k < 3; ++k) r.worst[k] = at[(size_t)k];
    r.sum_um = d[py::str("sum_um" + t)].cast<uint64_t>();
    r.p95_um = d[py::str("p95_um" + t)].cast<uint32_t>();
    r.found = d[py::str("found" + t)].cast<bool>() ? 1 : 0;
  }
  return c;
}

// A lesion-wise comparison record (nm03/volume_compare_lesions.h) as a dict: connectivity, max_lesions, the six
// totals, a_lesions / b_lesions (lists of dicts of the record's integers) and table (int64 [N + 1, N + 1]).
py::list volume_compare_lesion_list(const std::vector<VolumeCompareLesion>& v) {
  py::list out;
  for (const VolumeCompareLesion& r : v) {
    py::dict d;
    py::list at;
    for (int k = 0; k < 3; ++k) at.append(r.first[k]);
    d["voxels"] = r.voxels, d["first"] = at, d["overlap_vox"] = r.overlap_vox, d["partners_reported"] = r.partners_reported;
    d["overlap_other_vox"] = r.overlap_other_vox, d["multi"] = r.multi, d["best"] = r.best, d["best_overlap_vox"] = r.best_overlap_vox;
    out.append(d);
  }
  return out;
}

py::dict volume_compare_lesions_dict(const VolumeCompareLesions& l) {
  py::dict d;
  const VolumeCompareLesionsHead& hd = l.head;
  d["connectivity"] = hd.connectivity, d["max_lesions"] = hd.max_lesions;
  d["lesions_a"] = hd.lesions_a, d["hit_a"] = hd.hit_a, d["multi_a"] = hd.multi_a;
  d["lesions_b"] = hd.lesions_b, d["hit_b"] = hd.hit_b, d["multi_b"] = hd.multi_b;
  d["a_lesions"] = volume_compare_lesion_list(l.a);
  d["b_lesions"] = volume_compare_lesion_list(l.b);
  const int n1 = (int)hd.max_lesions + 1;
  std::vector<int64_t> t(l.table.begin(), l.table.end());
  d["table"] = to_np<int64_t>(t, {n1, n1});
  return d;
}

std::vector<VolumeCompareLesion> volume_compare_lesion_vector(const py::list& v) {
  std::vector<VolumeCompareLesion> out;
  for (const py::handle& hnd : v) {
    const py::dict d = py::reinterpret_borrow<py::dict>(hnd);
    VolumeCompareLesion r{};
    r.voxels = d["voxels"].cast<uint64_t>(), r.overlap_vox = d["overlap_vox"].cast<uint64_t>();
    r.overlap_other_vox = d["overlap_other_vox"].cast<uint64_t>(), r.best_overlap_vox = d["best_overlap_vox"].cast<uint64_t>();
    const std::vector<int> at = d["first"].cast<std::vector<int>>();
    if (at.size() != 3) throw std::invalid_argument("first must be [x, y, z]");
    for (int k = 0; k < 3; ++k) r.first[k] = at[(size_t)k];
    r.partners_reported = d["partners_reported"].cast<uint32_t>();
    r.multi = d["multi"].cast<int32_t>(), r.best = d["best"].cast<int32_t>();
    out.push_back(r);
  }
  return out;
}

VolumeCompareLesions volume_compare_lesions_from(const py::dict& d) {
  VolumeCompareLesions l;
  VolumeCompareLesionsHead& hd = l.head;
  hd.connectivity = d["connectivity"].cast<uint32_t>(), hd.max_lesions = d["max_lesions"].cast<uint32_t>();
  if (hd.max_lesions < 1 || hd.max_lesions > (uint32_t)kMaxVolumeLesions)
    throw std::invalid_argument("max_lesions must be 1.." + std::to_string(kMaxVolumeLesions));
  hd.lesions_a = d["lesions_a"].cast<uint32_t>(), hd.hit_a = d["hit_a"].cast<uint32_t>(), hd.multi_a = d["multi_a"].cast<uint32_t>();
  hd.lesions_b = d["lesions_b"].cast<uint32_t>(), hd.hit_b = d["hit_b"].cast<uint32_t>(), hd.multi_b = d["multi_b"].cast<uint32_t>();
  l.a = volume_compare_lesion_vector(d["a_lesions"].cast<py::list>());
  l.b = volume_compare_lesion_vector(d["b_lesions"].cast<py::list>());
  hd.reported_a = (uint32_t)l.a.size(), hd.reported_b = (uint32_t)l.b.size();
  const auto t = d["table"].cast<py::array_t<int64_t, py::array::c_style | py::array::forcecast>>();
  const size_t cells = (size_t)(hd.max_lesions + 1) * (hd.max_lesions + 1);
  if ((size_t)t.size() != cells) throw std::invalid_argument("table must be [max_lesions + 1, max_lesions + 1]");
  l.table.assign(t.data(), t.data() + cells);
  return l;
}

// The optional `lesions` argument of the writer bindings: None, or a lesion-wise comparison dict.
struct OptionalLesions {
  VolumeCompareLesions l;
  bool have = false;
  explicit OptionalLesions(const py::object& o) {
    if (!o.is_none()) l = volume_compare_lesions_from(o.cast<py::dict>()), have = true;
  }
  const VolumeCompareLesions* get() const { return have ? &l : nullptr; }
};

// The two masks of the comparison bindings: [D, H, W] of one shape.
void compare_args(const py::array& a, const py::array& b, const std::vector<int64_t>& spacing_um, uint32_t um[3]) {
  distance_args(a, spacing_um, um);
  if (b.ndim() != 3 || b.shape(0) != a.shape(0) || b.shape(1) != a.shape(1) || b.shape(2) != a.shape(2))
    throw std::invalid_argument("both masks must be [D, H, W] of one shape");
}

void check_max_lesions(int n) {
  if (n < 1 || n > kMaxVolumeLesions)
    throw std::invalid_argument("max_lesions must be 1.." + std::to_string(kMaxVolumeLesions));
}

// [D, H, W] 0/1 bytes → bit volume (d planes of h rows of ceil(w / 64) words, LSB = left-most voxel).
std::vector<uint64_t> pack_volume(const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& a) {
  const int d = (int)a.shape(0), h = (int)a.shape(1), w = (int)a.shape(2), wpr = (w + 63) / 64;
  std::vector<uint64_t> words((size_t)d * h * wpr, 0ull);
  const uint8_t* p = a.data();
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        if (p[((size_t)z * h + y) * w + x]) words[((size_t)z * h + y) * wpr + (x >> 6)] |= 1ull << (x & 63);
  return words;
}

// The fields of a volume beyond its samples that the Python surface passes to the 3D runner.
struct VolumeMeta {
  std::string type = "u16";
  int stored_bits = 16;
  float slope = 1.f, intercept = 0.f;
  std::vector<double> spacing = {1.0, 1.0, 1.0};  // x, y, z (mm)
  std::string spacing_z_source = "default";
  bool measure = false;
  int measure_connectivity = 26;
  int measure_lesions = 0;
  bool measure_diameters = false;
  bool measure_intensity = false;
  bool measure_texture = false;
  int texture_levels = 32;
  int64_t dilate_um = -1;  // ≥ 0: the margin in micrometres in place of the cube / ball
  bool measure_thickness = false;
  // VolumeRunner.run(compare_to=…): the reference mask [D, H, W] of a comparison and the name compare_json carries.
  bool compare = false;
  std::vector<uint8_t> compare_mask;
  int compare_shape[3] = {0, 0, 0};  // d, h, w
  std::string compare_reference;
  int compare_lesions = 0;  // VolumeRunner.run(compare_lesions=N): also the lesion-wise comparison (K18)
};

// compare_to of the runner bindings: None, or a [D, H, W] array (non-zero = set).
void compare_to_from(const py::object& o, const std::string& reference, VolumeMeta& mt) {
  if (o.is_none()) return;
  const auto a = o.cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>();
  if (a.ndim() != 3) throw std::invalid_argument("compare_to must be [D, H, W]");
  mt.compare = true;
  mt.compare_mask.assign(a.data(), a.data() + a.size());
  for (int k = 0; k < 3; ++k) mt.compare_shape[k] = (int)a.shape(k);
  mt.compare_reference = reference;
}

void apply_meta(const VolumeMeta& mt, VolumeInput& v) {
  if (mt.spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
  const PixelType t = parse_type(mt.type);
  v.type = t == kU8 ? kU16 : t;
  if (mt.stored_bits < 1 || mt.stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
  v.stored_bits = mt.stored_bits;
  v.slope = mt.slope;
  v.intercept = mt.intercept;
  v.spacing_x = (float)mt.spacing[0];
  v.spacing_y = (float)mt.spacing[1];
  v.spacing_z = mt.spacing[2];
  v.spacing_z_source = mt.spacing_z_source;
}

// --volume-views-at from Python: "mask", "centre", "X,Y,Z" or a sequence of three integers.
ViewsAt views_at_from(const py::object& o) {
  ViewsAt at;
  if (py::isinstance<py::str>(o)) {
    if (!views::parse_at(o.cast<std::string>(), &at)) throw std::invalid_argument("at must be 'mask', 'centre' or (x, y, z)");
    return at;
  }
  const auto p = o.cast<std::vector<int64_t>>();
  if (p.size() != 3) throw std::invalid_argument("at must be 'mask', 'centre' or (x, y, z)");
  for (int64_t c : p)
    if (c < -0x7FFFFFFFll || c > 0x7FFFFFFFll) throw std::invalid_argument("at: coordinate out of range");
  at.mode = kViewsAtPoint;
  at.x = (int)p[0], at.y = (int)p[1], at.z = (int)p[2];
  return at;
}

// A VolumeViews record as Python sees it: width, height, depth, at_mode, at, mask_bbox (None when the mask
// is empty), inverted and `views`, a dict name → {width, height, raw_min, raw_max, mask_px} plus the planes
// raw (uint16 [h, w]) and mask (uint8 [h, w]) when the record holds them.
py::dict views_dict(const VolumeViews& v) {
  py::dict d;
  d["width"] = v.w;
  d["height"] = v.h;
  d["depth"] = v.d;
  d["at_mode"] = std::string(views::at_mode_name(v.at_mode));
  d["at"] = py::make_tuple(v.at[0], v.at[1], v.at[2]);
  if (v.has_box) {
    py::list b;
    for (int k = 0; k < 6; ++k) b.append(v.box[k]);
    d["mask_bbox"] = b;
  } else {
    d["mask_bbox"] = py::none();
  }
  d["inverted"] = v.inverted;
  py::dict vs;
  for (int i = 0; i < kVolumeViewCount; ++i) {
    const VolumeView& q = v.view[i];
    py::dict e;
    e["width"] = q.w;
    e["height"] = q.h;
    e["raw_min"] = q.raw_min;
    e["raw_max"] = q.raw_max;
    e["mask_px"] = q.mask_px;
    if (!q.raw.empty()) e["raw"] = to_np<uint16_t>(q.raw, {q.h, q.w});
    if (!q.mask.empty()) e["mask"] = to_np<uint8_t>(q.mask, {q.h, q.w});
    vs[views::view_name(i)] = e;
  }
  d["views"] = vs;
  return d;
}

VolumeViews views_from(const py::dict& d) {
  VolumeViews v;
  v.w = d["width"].cast<int>();
  v.h = d["height"].cast<int>();
  v.d = d["depth"].cast<int>();
  const std::string mode = d["at_mode"].cast<std::string>();
  v.at_mode = mode == "mask" ? kViewsAtMask : mode == "centre" ? kViewsAtCentre : kViewsAtPoint;
  const auto at = d["at"].cast<std::vector<int>>();
  if (at.size() != 3) throw std::invalid_argument("views: at must be (x, y, z)");
  for (int a = 0; a < 3; ++a) v.at[a] = at[(size_t)a];
  v.has_box = !d["mask_bbox"].is_none();
  if (v.has_box) {
    const auto b = d["mask_bbox"].cast<std::vector<int>>();
    if (b.size() != 6) throw std::invalid_argument("views: mask_bbox must hold six integers");
    for (int a = 0; a < 6; ++a) v.box[a] = b[(size_t)a];
  }
  v.inverted = d["inverted"].cast<bool>();
  const py::dict vs = d["views"].cast<py::dict>();
  for (int i = 0; i < kVolumeViewCount; ++i) {
    const py::dict e = vs[views::view_name(i)].cast<py::dict>();
    VolumeView& q = v.view[i];
    q.w = e["width"].cast<int>();
    q.h = e["height"].cast<int>();
    q.raw_min = e["raw_min"].cast<int32_t>();
    q.raw_max = e["raw_max"].cast<int32_t>();
    q.mask_px = e["mask_px"].cast<uint32_t>();
    if (e.contains("raw")) q.raw = from_np<uint16_t>(e["raw"].cast<py::array_t<uint16_t, py::array::c_style | py::array::forcecast>>());
    if (e.contains("mask")) q.mask = from_np<uint8_t>(e["mask"].cast<py::array_t<uint8_t, py::array::c_style | py::array::forcecast>>());
  }
  return v;
}

py::dict view_files_dict(const std::vector<std::vector<uint8_t>>& files) {
  py::dict d;
  for (int k = 0; k < (int)files.size(); ++k)
    d[py::str(views::file_name(k / 2, k & 1))] = py::bytes((const char*)files[(size_t)k].data(), files[(size_t)k].size());
  return d;
}

// --volume-mesh-placement / -format from Python.
int mesh_placement_from(const std::string& s) {
  int p = kMeshCorner;
  if (!mesh::parse_placement(s, &p)) throw std::invalid_argument("placement must be 'corner' or 'nets'");
  return p;
}
int mesh_format_from(const std::string& s) {
  int f = kMeshPly;
  if (!mesh::parse_format(s, &f)) throw std::invalid_argument("format must be 'ply' or 'stl'");
  return f;
}

// A VolumeMesh as Python sees it: width, height, depth, placement, vertices (float32 [V, 3], mm), quads
// (int32 [Q, 4]), quads_x / _y / _z, voxels, k15_s.
py::dict mesh_dict(const VolumeMesh& m) {
  py::dict d;
  d["width"] = m.w;
  d["height"] = m.h;
  d["depth"] = m.d;
  d["placement"] = std::string(mesh::placement_name(m.placement));
  d["vertices"] = to_np<float>(m.positions, {(py::ssize_t)m.vertices(), 3});
  py::array_t<int32_t> q({(py::ssize_t)m.quad_count(), (py::ssize_t)4});
  if (!m.quads.empty()) std::memcpy(q.mutable_data(), m.quads.data(), m.quads.size() * 4);
  d["quads"] = q;
  d["quads_x"] = m.quads_x;
  d["quads_y"] = m.quads_y;
  d["quads_z"] = m.quads_z;
  d["voxels"] = m.voxels;
  d["k15_s"] = m.k15_s;
  return d;
}

VolumeMesh mesh_from(const py::dict& d) {
  VolumeMesh m;
  m.w = d["width"].cast<int>();
  m.h = d["height"].cast<int>();
  m.d = d["depth"].cast<int>();
  m.placement = mesh_placement_from(d["placement"].cast<std::string>());
  const auto v = d["vertices"].cast<py::array_t<float, py::array::c_style | py::array::forcecast>>();
  const auto q = d["quads"].cast<py::array_t<int32_t, py::array::c_style | py::array::forcecast>>();
  if (v.ndim() != 2 || v.shape(1) != 3 || q.ndim() != 2 || q.shape(1) != 4)
    throw std::invalid_argument("mesh: vertices must be [V, 3] and quads [Q, 4]");
  m.positions.assign(v.data(), v.data() + v.size());
  m.quads.resize((size_t)q.size());
  for (py::ssize_t i = 0; i < q.size(); ++i) {
    if (q.data()[i] < 0 || (size_t)q.data()[i] >= m.vertices()) throw std::invalid_argument("mesh: a quad index is not a vertex");
    m.quads[(size_t)i] = (uint32_t)q.data()[i];
  }
  m.quads_x = d["quads_x"].cast<uint64_t>();
  m.quads_y = d["quads_y"].cast<uint64_t>();
  m.quads_z = d["quads_z"].cast<uint64_t>();
  m.voxels = d["voxels"].cast<uint64_t>();
  return m;
}

}  // namespace

template <class Fn>
py::dict volume_call(py::array_t<uint16_t, py::array::c_style | py::array::forcecast> vol, const PipelineParams& p,
                     int connectivity, int dilation, const std::vector<std::tuple<int, int, int>>& seeds, Fn&& fn,
                     const VolumeMeta* meta = nullptr) {
  if (vol.ndim() != 3) throw std::invalid_argument("volume must be (depth, height, width)");
  VolumeInput v;
  v.d = (int)vol.shape(0);
  v.h = (int)vol.shape(1);
  v.w = (int)vol.shape(2);
  v.raw = from_np<uint16_t>(vol);
  VolumeParams vp;
  vp.pipe = p;
  vp.connectivity = connectivity;
  vp.dilation_size = dilation;
  vp.seeds = seeds_from(seeds);
  if (meta) {
    apply_meta(*meta, v);
    vp.measure = meta->measure;
    vp.measure_connectivity = meta->measure_connectivity;
    vp.measure_lesions = meta->measure_lesions;
    vp.measure_diameters = meta->measure_diameters;
    // The spacing the lengths are maximised in: the sidecar's (float pixel spacings), in integer micrometres.
    if (vp.measure_diameters) measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
    vp.measure_intensity = meta->measure_intensity;
    vp.measure_texture = meta->measure_texture;
    vp.texture_levels = meta->texture_levels;
    vp.dilate_um = meta->dilate_um;
    vp.measure_thickness = meta->measure_thickness;
    if (vp.dilate_um >= 0 || vp.measure_thickness || meta->compare)
      measure::volume_spacing_um((double)v.spacing_x, (double)v.spacing_y, v.spacing_z, vp.spacing_um);
  }
  VolumeReference ref;
  if (meta && meta->compare) {
    ref.mask = meta->compare_mask.data();
    ref.d = meta->compare_shape[0], ref.h = meta->compare_shape[1], ref.w = meta->compare_shape[2];
    vp.compare = &ref;
  }
  if (meta) vp.compare_lesions = meta->compare_lesions;  // checked by the runner (needs compare_to, 1 … 64)
  VolumeResult r;
  {
    py::gil_scoped_release nogil;
    r = fn(v, vp);
  }
  py::dict d;
  d["band"] = to_np<uint8_t>(r.band, {v.d, v.h, v.w});
  d["region"] = to_np<uint8_t>(r.region, {v.d, v.h, v.w});
  d["dilated"] = to_np<uint8_t>(r.dilated, {v.d, v.h, v.w});
  d["sweeps"] = r.sweeps;
  d["kernels_s"] = r.kernels_s;
  if (vp.measure) {
    d["measure"] = volume_measure_dict(r.measure);
    d["measure_json"] = golden::measure_volume_json(r.measure, v, vp.pipe.apply_rescale, vp.measure_connectivity);
    if (vp.measure_lesions) {
      d["lesions"] = volume_lesion_list(r.lesions.data(), r.lesions.size());
      d["measure_json"] = golden::measure_volume_json(r.measure, r.lesions, vp.measure_lesions, v, vp.pipe.apply_rescale,
                                                      vp.measure_connectivity);
    }
    if (vp.measure_intensity) {
      d["intensity"] = intensity_dict(r.intensity);
      d["measure_json"] = golden::measure_volume_json(r.measure, r.intensity, vp.measure_lesions ? &r.lesions : nullptr,
                                                      vp.measure_lesions, v, vp.pipe.apply_rescale, vp.measure_connectivity);
    }
    if (vp.measure_texture) {
      d["texture"] = texture_dict(r.texture);
      d["measure_json"] = golden::measure_volume_json(r.measure, vp.measure_intensity ? &r.intensity : nullptr,
                                                      vp.measure_lesions ? &r.lesions : nullptr, vp.measure_lesions, r.texture, v,
                                                      vp.pipe.apply_rescale, vp.measure_connectivity);
    }
    if (vp.measure_thickness) {
      d["thickness"] = volume_thickness_dict(r.thickness);
      d["measure_json"] = measure::insert_thickness_keys(d["measure_json"].cast<std::string>(), r.thickness, vp.spacing_um);
    }
    if (vp.measure_diameters) {
      d["diameters"] = volume_diameters_list(r.diameters.data(), r.diameters.size());
      d["measure_json"] = measure::insert_diameter_keys(d["measure_json"].cast<std::string>(), r.diameters.data(),
                                                        (int)r.diameters.size(), vp.spacing_um);
    }
    d["measure_s"] = r.measure_s;
  }
  if (vp.compare) {
    d["compare"] = volume_compare_dict(r.compare);
    d["compare_json"] = compare::to_json(r.compare, v.w, v.h, v.d, vp.spacing_um, meta->compare_reference,
                                         vp.compare_lesions ? &r.compare_lesions : nullptr);
    d["compare_s"] = r.compare_s;
    if (vp.compare_lesions) {
      d["compare_lesions"] = volume_compare_lesions_dict(r.compare_lesions);
      d["compare_lesions_s"] = r.compare_lesions_s;
    }
  }
  return d;
}

PYBIND11_MODULE(_nm03, m) {
  m.doc() = "NM03 MI355X-native DICOM batch engine (native core)";

  // ---- parameters -----------------------------------------------------------------------------
  py::class_<PipelineParams>(m, "PipelineParams")
      .def(py::init<>())
      .def_readwrite("norm_low", &PipelineParams::norm_low)
      .def_readwrite("norm_high", &PipelineParams::norm_high)
      .def_readwrite("norm_min", &PipelineParams::norm_min)
      .def_readwrite("norm_max", &PipelineParams::norm_max)
      .def_readwrite("clip_min", &PipelineParams::clip_min)
      .def_readwrite("clip_max", &PipelineParams::clip_max)
      .def_readwrite("median_window", &PipelineParams::median_window)
      .def_readwrite("sharpen_gain", &PipelineParams::sharpen_gain)
      .def_readwrite("sharpen_sigma", &PipelineParams::sharpen_sigma)
      .def_readwrite("sharpen_mask", &PipelineParams::sharpen_mask)
      .def_readwrite("srg_min", &PipelineParams::srg_min)
      .def_readwrite("srg_max", &PipelineParams::srg_max)
      .def_readwrite("srg_connectivity", &PipelineParams::srg_connectivity)
      .def_readwrite("dilation_size", &PipelineParams::dilation_size)
      .def_readwrite("erosion_size", &PipelineParams::erosion_size)
      .def_readwrite("min_dim", &PipelineParams::min_dim)
      .def_readwrite("apply_rescale", &PipelineParams::apply_rescale)
      .def_readwrite("frame", &PipelineParams::frame)
      .def_readwrite("se_shape", &PipelineParams::se_shape)
      .def_readwrite("measure", &PipelineParams::measure)
      .def_readwrite("measure_diameters", &PipelineParams::measure_diameters)
      .def_readwrite("measure_intensity", &PipelineParams::measure_intensity)
      .def_readwrite("measure_texture", &PipelineParams::measure_texture)
      .def_readwrite("texture_levels", &PipelineParams::texture_levels)
      .def_property(
          "measure_connectivity", [](const PipelineParams& p) { return (int)p.measure_connectivity; },
          [](PipelineParams& p, int v) {
            if (v != 4 && v != 8) throw std::invalid_argument("measure_connectivity must be 4 or 8");
            p.measure_connectivity = (uint8_t)v;
          });
  py::class_<RenderParams>(m, "RenderParams")
      .def(py::init<>())
      .def_readwrite("out_width", &RenderParams::out_width)
      .def_readwrite("out_height", &RenderParams::out_height)
      .def_readwrite("label_opacity", &RenderParams::label_opacity)
      .def_readwrite("border_opacity", &RenderParams::border_opacity)
      .def_readwrite("border_radius", &RenderParams::border_radius)
      .def_readwrite("jpeg_quality", &RenderParams::jpeg_quality)
      .def_readwrite("filter", &RenderParams::filter)
      .def_readwrite("jpeg_sampling", &RenderParams::jpeg_sampling)
      .def_readwrite("overlay", &RenderParams::overlay)
      .def_property(
          "overlay_color",
          [](const RenderParams& r) { return py::make_tuple(r.overlay_color[0], r.overlay_color[1], r.overlay_color[2]); },
          [](RenderParams& r, const std::vector<int>& c) {
            if (c.size() != 3) throw std::invalid_argument("overlay_color must have three values 0..255");
            for (int v : c)
              if (v < 0 || v > 255) throw std::invalid_argument("overlay_color must have three values 0..255");
            for (int k = 0; k < 3; ++k) r.overlay_color[k] = (uint8_t)c[k];
          });
  py::class_<EngineConfig>(m, "EngineConfig")
      .def(py::init<>())
      .def_readwrite("device", &EngineConfig::device)
      .def_readwrite("batch_size", &EngineConfig::batch_size)
      .def_readwrite("streams", &EngineConfig::streams)
      .def_readwrite("threads", &EngineConfig::threads)
      .def_readwrite("cpus", &EngineConfig::cpus)
      .def_readwrite("max_dim", &EngineConfig::max_dim)
      .def_readwrite("pipe", &EngineConfig::pipe)
      .def_readwrite("render", &EngineConfig::render)
      .def_readwrite("export_jpeg", &EngineConfig::export_jpeg)
      .def_readwrite("resume", &EngineConfig::resume)
      .def_readwrite("jpeg_out_cap", &EngineConfig::jpeg_out_cap)
      .def_readwrite("upload_chunk_kb", &EngineConfig::upload_chunk_kb)
      .def_readwrite("create_writers", &EngineConfig::create_writers)
      .def_readwrite("lazy_slots", &EngineConfig::lazy_slots)
      .def_readwrite("host_only", &EngineConfig::host_only);

  m.def("reference_seeds", [](int w, int h) {
    std::vector<std::pair<int, int>> v;
    for (auto& s : reference_seeds(w, h)) v.push_back({s.x, s.y});
    return v;
  });
  m.def("gaussian_taps", [](float sigma, int mask) {
    std::vector<float> t(mask);
    gaussian_taps(sigma, mask, t.data());
    return t;
  });

  // ---- DICOM -----------------------------------------------------------------------------------
  m.def("dicom_parse", [](py::bytes b) {
    std::string s = b;
    return header_dict(dicom::parse((const uint8_t*)s.data(), s.size()));
  });
  m.def(
      "dicom_pixels",
      [](py::bytes b, int frame) {
        std::string s = b;
        dicom::Header h = dicom::parse((const uint8_t*)s.data(), s.size());
        std::vector<uint16_t> px((size_t)h.rows * h.cols);
        dicom::copy_pixels16(h, (const uint8_t*)s.data(), s.size(), px.data(), frame);
        return to_np<uint16_t>(px, {h.rows, h.cols});
      },
      py::arg("data"), py::arg("frame") = 0);
  m.def("dicom_select_frame", [](py::bytes b, int policy) {
    std::string s = b;
    return dicom::select_frame(dicom::parse((const uint8_t*)s.data(), s.size()), policy);
  });
  m.def(
      "dicom_bytes",
      [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> px, const std::string& type, int bits_stored,
         bool write_rescale, float slope, float intercept, float sx, float sy, int instance, const std::string& patient_id,
         const std::string& syntax, bool preamble, const std::string& photometric, int jpeg_predictor,
         int jpeg_restart_rows, int jpeg_fragments, int jpeg_quality, double slice_thickness,
         double spacing_between_slices, const std::vector<double>& position, bool write_position) {
        dicom::WriteSpec w;
        w.slice_thickness = slice_thickness;
        w.spacing_between_slices = spacing_between_slices;
        if (position.size() != 3) throw std::invalid_argument("position must be (x, y, z)");
        for (int k = 0; k < 3; ++k) w.position[k] = position[(size_t)k];
        w.write_position = write_position;
        w.jpeg_quality = jpeg_quality;
        w.jpeg_predictor = jpeg_predictor;
        w.jpeg_restart_rows = jpeg_restart_rows;
        w.jpeg_fragments = jpeg_fragments;
        // (rows, cols) or (frames, rows, cols)
        if (px.ndim() != 2 && px.ndim() != 3) throw std::invalid_argument("pixels must be 2D or 3D (frames, rows, cols)");
        w.frames = px.ndim() == 3 ? (int)px.shape(0) : 1;
        w.rows = (int)px.shape(px.ndim() - 2);
        w.cols = (int)px.shape(px.ndim() - 1);
        w.photometric = photometric;
        w.type = parse_type(type);
        w.bits_stored = bits_stored;
        std::vector<uint16_t> v = from_np<uint16_t>(px);
        w.pixels = v.data();
        w.write_rescale = write_rescale;
        w.slope = slope;
        w.intercept = intercept;
        w.spacing_x = sx;
        w.spacing_y = sy;
        w.instance_number = instance;
        w.patient_id = patient_id;
        w.syntax = syntax == "implicit"   ? dicom::Syntax::kImplicitLE
                   : syntax == "big"      ? dicom::Syntax::kExplicitBE
                   : syntax == "deflated" ? dicom::Syntax::kDeflatedLE
                   : syntax == "rle"      ? dicom::Syntax::kRleLossless
                   : syntax == "jpeg-lossless" ? dicom::Syntax::kJpegLossless
                   : syntax == "jpeg-baseline" ? dicom::Syntax::kJpegBaseline
                   : syntax == "jpeg-extended" ? dicom::Syntax::kJpegExtended
                   : syntax == "explicit" ? dicom::Syntax::kExplicitLE
                                          : throw std::invalid_argument("syntax: implicit|explicit|big|deflated|rle|jpeg-lossless|jpeg-baseline|jpeg-extended");
        w.preamble = preamble;
        auto b = dicom::write(w);
        return py::bytes((const char*)b.data(), b.size());
      },
      py::arg("pixels"), py::arg("type") = "u16", py::arg("bits_stored") = 16, py::arg("write_rescale") = false,
      py::arg("slope") = 1.f, py::arg("intercept") = 0.f, py::arg("spacing_x") = 1.f, py::arg("spacing_y") = 1.f,
      py::arg("instance") = 1, py::arg("patient_id") = "PGBM-000", py::arg("syntax") = "explicit",
      py::arg("preamble") = true, py::arg("photometric") = "MONOCHROME2", py::arg("jpeg_predictor") = 1,
      py::arg("jpeg_restart_rows") = 0, py::arg("jpeg_fragments") = 1, py::arg("jpeg_quality") = 90,
      py::arg("slice_thickness") = 1.0, py::arg("spacing_between_slices") = 0.0,
      py::arg("position") = std::vector<double>{0.0, 0.0, 0.0}, py::arg("write_position") = true);
  // Geometry of a series from the headers of its first two files: PixelSpacing and the plane spacing
  // with its source (position | spacing_between_slices | slice_thickness | default), as load_volume sets them.
  m.def("series_geometry", [](const std::vector<std::string>& files) {
    const SeriesGeometry g = series_geometry(files);
    py::dict d;
    d["spacing_x"] = g.spacing_x;
    d["spacing_y"] = g.spacing_y;
    d["spacing_z"] = g.spacing_z;
    d["spacing_z_source"] = g.spacing_z_source;
    return d;
  }, py::arg("files"));
  m.def("jpeg_dct_decode", [](py::bytes b) {
    const std::string s = b;
    std::vector<uint16_t> px;
    const jpegdct::Info i = jpegdct::decode((const uint8_t*)s.data(), s.size(), px);
    py::dict d;
    d["precision"] = i.precision;
    d["sof"] = i.sof;
    d["restart_interval"] = i.restart_interval;
    d["pixels"] = to_np(px, {(py::ssize_t)i.rows, (py::ssize_t)i.cols});
    return d;
  });
  m.def("jpeg_dct_encode", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> px, int precision,
                              int quality, int restart_blocks) {
    if (px.ndim() != 2) throw std::invalid_argument("pixels must be 2D");
    std::vector<uint16_t> v = from_np<uint16_t>(px);
    auto j = jpegdct::encode(v.data(), (int)px.shape(0), (int)px.shape(1), precision, quality, restart_blocks);
    return py::bytes((const char*)j.data(), j.size());
  }, py::arg("pixels"), py::arg("precision") = 8, py::arg("quality") = 90, py::arg("restart_blocks") = 0);
  m.def("jpeg_lossless_decode", [](py::bytes b) {
    const std::string s = b;
    std::vector<uint16_t> px;
    const jpegll::Info i = jpegll::decode((const uint8_t*)s.data(), s.size(), px);
    py::dict d;
    d["precision"] = i.precision;
    d["predictor"] = i.predictor;
    d["point_transform"] = i.point_transform;
    d["restart_interval"] = i.restart_interval;
    d["pixels"] = to_np(px, {(py::ssize_t)i.rows, (py::ssize_t)i.cols});
    return d;
  });
  m.def("jpeg_lossless_encode", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> px, int precision,
                                   int predictor, int pt, int restart_rows) {
    if (px.ndim() != 2) throw std::invalid_argument("pixels must be 2D");
    std::vector<uint16_t> v = from_np<uint16_t>(px);
    auto j = jpegll::encode(v.data(), (int)px.shape(0), (int)px.shape(1), precision, predictor, pt, restart_rows);
    return py::bytes((const char*)j.data(), j.size());
  }, py::arg("pixels"), py::arg("precision") = 16, py::arg("predictor") = 1, py::arg("pt") = 0, py::arg("restart_rows") = 0);
  m.def("numa_parse_cpulist", &numa::parse_cpulist);
  m.def(
      "mhd_write",
      [](const std::string& base, py::array arr, float sx, float sy, float sz) {
        py::buffer_info bi = arr.request();
        if (!(py::array::c_style & arr.flags())) throw std::invalid_argument("array must be C-contiguous");
        mhd::MetType t;
        const std::string f = bi.format;
        if (bi.itemsize == 1) t = mhd::MetType::kUChar;
        else if (bi.itemsize == 2 && (f == "H")) t = mhd::MetType::kUShort;
        else if (bi.itemsize == 2 && (f == "h")) t = mhd::MetType::kShort;
        else if (bi.itemsize == 4 && f == "f") t = mhd::MetType::kFloat;
        else throw std::invalid_argument("mhd_write: uint8, uint16, int16 or float32 arrays only");
        int w = 1, h = 1, d = 1;
        if (bi.ndim == 2) { h = (int)bi.shape[0]; w = (int)bi.shape[1]; }
        else if (bi.ndim == 3) { d = (int)bi.shape[0]; h = (int)bi.shape[1]; w = (int)bi.shape[2]; }
        else throw std::invalid_argument("mhd_write: 2D or 3D arrays only");
        mhd::write(base, bi.ptr, w, h, d, t, sx, sy, sz);
      },
      py::arg("base"), py::arg("array"), py::arg("sx") = 1.f, py::arg("sy") = 1.f, py::arg("sz") = 1.f);
  m.def("mhd_read", [](const std::string& path) {
    mhd::Image im = mhd::read(path);
    std::vector<py::ssize_t> shape = im.d > 1 ? std::vector<py::ssize_t>{im.d, im.h, im.w}
                                               : std::vector<py::ssize_t>{im.h, im.w};
    py::array a;
    switch (im.type) {
      case mhd::MetType::kUChar: a = py::array_t<uint8_t>(shape); break;
      case mhd::MetType::kUShort: a = py::array_t<uint16_t>(shape); break;
      case mhd::MetType::kShort: a = py::array_t<int16_t>(shape); break;
      case mhd::MetType::kFloat: a = py::array_t<float>(shape); break;
    }
    std::memcpy(a.mutable_data(), im.bytes.data(), im.bytes.size());
    return py::make_tuple(a, py::make_tuple(im.spacing[0], im.spacing[1], im.spacing[2]));
  });
  m.def("numa_node_cpus", &numa::node_cpus);
  m.def("numa_device_node", &numa::device_node, py::arg("device"));
  m.def("device_bus_id", &numa::device_bus_id, py::arg("device"));
  m.def("cpu_budget", &numa::cpu_budget, py::arg("cgroup_root") = "/sys/fs/cgroup");
  m.def("allowed_cpus", &numa::allowed_cpus);
  m.def("format_cpulist", &numa::format_cpulist);
  // Per-rank CPU partition (numa.h): {node, index, count, cpus, threads}. `sysfs` / `allowed` let
  // tests describe a fake host.
  m.def(
      "rank_partition",
      [](const std::vector<int>& rank_nodes, int local_rank, int budget, int cap, const std::string& sysfs,
         const std::vector<int>& allowed) {
        const numa::Topology t = numa::read_topology(sysfs, allowed);
        const numa::RankCpus r = numa::rank_partition(t, rank_nodes, local_rank, budget, cap);
        py::dict d;
        d["node"] = r.node;
        d["index"] = r.index;
        d["count"] = r.count;
        d["cpus"] = r.cpus;
        d["threads"] = r.threads;
        return d;
      },
      py::arg("rank_nodes"), py::arg("local_rank"), py::arg("budget"), py::arg("cap") = 16,
      py::arg("sysfs") = "/sys", py::arg("allowed") = std::vector<int>{});
  m.def(
      "read_pixels_direct",
      [](const std::string& path, const std::string& mode, size_t prefix, int frame) {
        dicom::SliceFile f(path, mode == "staged" ? dicom::ReadMode::kStaged : dicom::ReadMode::kDirect, prefix);
        std::vector<uint8_t> scratch;
        const dicom::Header& h = f.header(scratch);
        std::vector<uint16_t> px((size_t)h.rows * h.cols + 1);  // +1: misaligned destination below
        uint16_t* dst = px.data() + 1;
        f.pixels16(dst, frame);
        std::vector<uint16_t> out(dst, dst + (size_t)h.rows * h.cols);
        // The staged fast path's view of the same frame (None when pixels16 must convert).
        const uint16_t* ss = f.staged_samples(frame);
        py::object staged = py::none();
        if (ss) staged = to_np<uint16_t>(std::vector<uint16_t>(ss, ss + (size_t)h.rows * h.cols), {h.rows, h.cols});
        return py::make_tuple(to_np<uint16_t>(out, {h.rows, h.cols}), f.direct(), staged);
      },
      py::arg("path"), py::arg("mode") = "direct", py::arg("prefix") = 16384, py::arg("frame") = 0);
  m.def(
      "read_slice",
      [](const std::string& path, int min_dim, int frame) {
        golden::SliceInput s = golden::load_slice(path, min_dim, frame);
        py::dict meta;
        meta["type"] = s.type == kI16 ? "i16" : "u16";
        meta["stored_bits"] = s.stored_bits;
        meta["slope"] = s.slope;
        meta["intercept"] = s.intercept;
        meta["spacing_x"] = s.spacing_x;
        meta["spacing_y"] = s.spacing_y;
        return py::make_tuple(to_np<uint16_t>(s.raw, {s.h, s.w}), meta);
      },
      py::arg("path"), py::arg("min_dim") = 0, py::arg("frame") = -1);

  // ---- cohort / synthetic data -------------------------------------------------------------------
  m.def("extract_file_number", &cohort::extract_file_number);
  // img_processing_parallel's default rank count (app.h): policy and the listing-only slice count.
  m.def("auto_gpus", &app::auto_gpus, py::arg("slices"), py::arg("visible"));
  m.def("auto_slices_per_rank", [] { return app::kAutoSlicesPerRank; });
  m.def("count_cohort_slices", [](const std::string& data_root) {
    app::AppConfig c;
    c.data_root = cohort::with_slash(data_root);
    return app::count_cohort_slices(c);
  });
  m.def("default_data_root", &cohort::default_data_root);
  m.def("cohort_dir", &cohort::cohort_dir);
  m.def("test_slice_path", &cohort::test_slice_path);
  m.def("find_patient_dirs", &cohort::find_patient_dirs);
  m.def("list_patient_series", [](const std::string& root, const std::string& pid) {
    auto s = cohort::list_patient_series(root, pid);
    return py::make_tuple(s.series_dir, s.files);
  });
  m.def("setup_output_dir", &cohort::setup_output_dir);
  m.def("setup_output_dirs", [](const std::vector<std::string>& dirs, int threads) {
    py::gil_scoped_release nogil;
    cohort::setup_output_dirs(dirs, threads);
  }, py::arg("dirs"), py::arg("threads") = 8);
  py::class_<cohort::OutputReaper>(m, "OutputReaper")
      .def(py::init<int>(), py::arg("threads") = 4)
      .def("wipe", [](cohort::OutputReaper& r, const std::vector<std::string>& dirs) {
        py::gil_scoped_release nogil;
        r.wipe(dirs);
      })
      .def("drain", [](cohort::OutputReaper& r) {
        py::gil_scoped_release nogil;
        r.drain();
      })
      .def_property_readonly("files_reaped", &cohort::OutputReaper::files_reaped);
  m.def(
      "synth_cohort",
      [](const std::string& root, int patients, int min_slices, int max_slices, int rows, int cols, uint64_t seed,
         int threads, bool test_slice, bool decoy, bool signed_px) {
        synth::CohortSpec s;
        s.data_root = cohort::with_slash(root);
        s.patients = patients;
        s.min_slices = min_slices;
        s.max_slices = max_slices;
        s.rows = rows;
        s.cols = cols;
        s.seed = seed;
        s.threads = threads;
        s.test_slice = test_slice;
        s.decoy_series = decoy;
        s.type = signed_px ? kI16 : kU16;
        py::gil_scoped_release nogil;
        return synth::generate_cohort(s);
      },
      py::arg("data_root"), py::arg("patients") = 20, py::arg("min_slices") = 21, py::arg("max_slices") = 25,
      py::arg("rows") = 256, py::arg("cols") = 256, py::arg("seed") = 20250404, py::arg("threads") = 8,
      py::arg("test_slice") = true, py::arg("decoy") = false, py::arg("signed") = false);
  m.def("synth_flat", [](const std::string& root, int count, int rows, int cols, uint64_t seed, int threads) {
    py::gil_scoped_release nogil;
    return synth::generate_flat(root, count, rows, cols, seed, threads);
  });
  m.def("phantom_slice", [](int rows, int cols, int patient, int slice, int nslices, uint64_t seed) {
    std::vector<uint16_t> v((size_t)rows * cols);
    synth::phantom_slice(rows, cols, patient, slice, nslices, seed, v.data());
    return to_np<uint16_t>(v, {rows, cols});
  });

  // ---- golden model ----------------------------------------------------------------------------
  m.def(
      "golden_run",
      [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type, int stored_bits,
         float slope, float intercept, const PipelineParams& p, const RenderParams& rp, float sx, float sy) {
        golden::SliceInput s = slice_from(raw, type, stored_bits, slope, intercept, sx, sy);
        golden::SliceResult r = golden::run(s, p, true);
        py::dict d;
        d["clipped"] = to_np<float>(r.clipped, {s.h, s.w});
        d["median"] = to_np<float>(r.median, {s.h, s.w});
        d["sharpened"] = to_np<float>(r.sharpened, {s.h, s.w});
        d["band"] = mask2d(r.band, s.h, s.w);
        d["region"] = mask2d(r.region, s.h, s.w);
        d["eroded"] = mask2d(r.eroded, s.h, s.w);
        d["dilated"] = mask2d(r.dilated, s.h, s.w);
        d["window"] = py::make_tuple(r.window_lo, r.window_hi);
        golden::SliceJpegs j = golden::export_jpegs(s, r, p, rp);
        d["jpeg_original"] = py::bytes((const char*)j.original.data(), j.original.size());
        d["jpeg_processed"] = py::bytes((const char*)j.processed.data(), j.processed.size());
        if (rp.overlay) {
          d["overlay"] = to_np<uint8_t>(j.overlay_canvas, {rp.out_height, rp.out_width, 3});
          d["jpeg_overlay"] = py::bytes((const char*)j.overlay.data(), j.overlay.size());
        }
        if (p.measure || p.measure_diameters || p.measure_intensity || p.measure_texture) {
          const SliceMeasure sm = golden::measure(r.dilated, r.region, s, p.measure_connectivity);
          d["measure"] = measure_dict(sm);
          if (p.measure_intensity) d["intensity"] = intensity_dict(golden::measure_intensity(r.dilated, s));
          if (p.measure_diameters) {
            const SliceDiameters sd = golden::measure_diameters(r.dilated, p.measure_connectivity, s.w, s.h);
            d["diameters"] = diameters_dict(sd);
            d["measure_json"] = golden::measure_json(sm, sd, s, p);
          } else {
            d["measure_json"] = golden::measure_json(sm, s, p);
          }
          if (p.measure_intensity || p.measure_texture) d["measure_json"] = golden::measure_sidecar(r.dilated, r.region, s, p);
          if (p.measure_texture) d["texture"] = texture_dict(golden::measure_texture(r.dilated, s, p.texture_levels));
        }
        return d;
      },
      py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("slope") = 1.f,
      py::arg("intercept") = 0.f, py::arg("params") = PipelineParams(), py::arg("render") = RenderParams(),
      py::arg("spacing_x") = 1.f, py::arg("spacing_y") = 1.f);
  m.def("golden_norm_clip", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                               int stored_bits, float slope, float intercept, const PipelineParams& p) {
    golden::SliceInput s = slice_from(raw, type, stored_bits, slope, intercept, 1, 1);
    return to_np<float>(golden::norm_clip(s, p), {s.h, s.w});
  });
  m.def("golden_median", [](py::array_t<float, py::array::c_style | py::array::forcecast> img, int k) {
    const int h = (int)img.shape(0), w = (int)img.shape(1);
    return to_np<float>(golden::median(from_np<float>(img), w, h, k), {h, w});
  });
  m.def("golden_median_u16", [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> img, int k) {
    const int h = (int)img.shape(0), w = (int)img.shape(1);
    return to_np<uint16_t>(golden::median_u16(from_np<uint16_t>(img), w, h, k), {h, w});
  });
  m.def("golden_vector_median", [](py::array_t<float, py::array::c_style | py::array::forcecast> img, int k) {
    const int h = (int)img.shape(0), w = (int)img.shape(1);
    return to_np<float>(golden::vector_median(from_np<float>(img), w, h, k), {h, w});
  });
  m.def("golden_sharpen", [](py::array_t<float, py::array::c_style | py::array::forcecast> img, float gain, float sigma,
                             int mask, bool direct) {
    const int h = (int)img.shape(0), w = (int)img.shape(1);
    auto v = from_np<float>(img);
    return to_np<float>(direct ? golden::sharpen_direct(v, w, h, gain, sigma, mask) : golden::sharpen(v, w, h, gain, sigma, mask),
                        {h, w});
  }, py::arg("img"), py::arg("gain") = 2.0f, py::arg("sigma") = 0.5f, py::arg("mask") = 9, py::arg("direct") = false);
  m.def("golden_region_grow", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> band,
                                 const std::vector<std::tuple<int, int, int>>& seeds, int conn) {
    const int h = (int)band.shape(0), w = (int)band.shape(1);
    return mask2d(golden::region_grow(from_np<uint8_t>(band), w, h, seeds_from(seeds), conn), h, w);
  });
  m.def(
      "golden_morph",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mk, int size, bool dilate, bool disc) {
        const int h = (int)mk.shape(0), w = (int)mk.shape(1);
        auto v = from_np<uint8_t>(mk);
        return mask2d(dilate ? golden::dilate(v, w, h, size, disc) : golden::erode(v, w, h, size, disc), h, w);
      },
      py::arg("mask"), py::arg("size"), py::arg("dilate"), py::arg("disc") = false);
  m.def("golden_border", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mk, int radius) {
    const int h = (int)mk.shape(0), w = (int)mk.shape(1);
    return mask2d(golden::border(from_np<uint8_t>(mk), w, h, radius), h, w);
  });
  m.def("golden_region_grow3d", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> band,
                                   const std::vector<std::tuple<int, int, int>>& seeds, int conn) {
    const int d = (int)band.shape(0), h = (int)band.shape(1), w = (int)band.shape(2);
    return to_np<uint8_t>(golden::region_grow3d(from_np<uint8_t>(band), w, h, d, seeds_from(seeds), conn), {d, h, w});
  });
  m.def(
      "golden_dilate3d",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mk, int size, bool ball) {
        const int d = (int)mk.shape(0), h = (int)mk.shape(1), w = (int)mk.shape(2);
        return to_np<uint8_t>(golden::dilate3d(from_np<uint8_t>(mk), w, h, d, size, ball), {d, h, w});
      },
      py::arg("mask"), py::arg("size"), py::arg("ball") = false);
  m.def(
      "golden_render_gray",
      [](py::array_t<float, py::array::c_style | py::array::forcecast> v, float lo, float hi, float sx, float sy, int out_w,
         int out_h, bool nearest) {
        const int h = (int)v.shape(0), w = (int)v.shape(1);
        RenderGeom g = make_render_geom(w, h, sx, sy, out_w, out_h);
        return to_np<uint8_t>(golden::render_gray(from_np<float>(v), g, lo, hi, nearest), {out_h, out_w});
      },
      py::arg("values"), py::arg("lo"), py::arg("hi"), py::arg("sx"), py::arg("sy"), py::arg("out_w"), py::arg("out_h"),
      py::arg("nearest") = false);
  m.def("golden_render_labels", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> lab,
                                   py::array_t<uint8_t, py::array::c_style | py::array::forcecast> brd, float sx, float sy,
                                   int out_w, int out_h, int fill, int bv) {
    const int h = (int)lab.shape(0), w = (int)lab.shape(1);
    RenderGeom g = make_render_geom(w, h, sx, sy, out_w, out_h);
    return to_np<uint8_t>(golden::render_labels(from_np<uint8_t>(lab), from_np<uint8_t>(brd), g, (uint8_t)fill, (uint8_t)bv),
                          {out_h, out_w});
  });
  m.def(
      "golden_render_overlay",
      [](py::array_t<float, py::array::c_style | py::array::forcecast> v,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> lab,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> brd, float lo, float hi, float sx, float sy,
         int out_w, int out_h, bool nearest, int fill_a, int border_a, const std::vector<int>& color) {
        const int h = (int)v.shape(0), w = (int)v.shape(1);
        if (lab.ndim() != 2 || brd.ndim() != 2 || lab.shape(0) != h || lab.shape(1) != w || brd.shape(0) != h ||
            brd.shape(1) != w)
          throw std::invalid_argument("label and border must have the shape of values");
        if (color.size() != 3) throw std::invalid_argument("color must have three values");
        const uint8_t c[3] = {(uint8_t)color[0], (uint8_t)color[1], (uint8_t)color[2]};
        RenderGeom g = make_render_geom(w, h, sx, sy, out_w, out_h);
        return to_np<uint8_t>(golden::render_overlay(from_np<float>(v), from_np<uint8_t>(lab), from_np<uint8_t>(brd), g, lo,
                                                     hi, nearest, (uint8_t)fill_a, (uint8_t)border_a, c),
                              {out_h, out_w, 3});
      },
      py::arg("values"), py::arg("label"), py::arg("border"), py::arg("lo"), py::arg("hi"), py::arg("sx") = 1.f,
      py::arg("sy") = 1.f, py::arg("out_w") = 512, py::arg("out_h") = 512, py::arg("nearest") = false,
      py::arg("fill_a") = 153, py::arg("border_a") = 255, py::arg("color") = std::vector<int>{0, 255, 0});
  m.def("opacity_u8", &opacity_u8);

  // ---- measurements (nm03/measure.h) -----------------------------------------------------------------
  m.def(
      "golden_measure",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> reg,
         py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type, int stored_bits,
         int connectivity) {
        if (dil.ndim() != 2 || reg.ndim() != 2 || raw.ndim() != 2 || reg.shape(0) != dil.shape(0) ||
            reg.shape(1) != dil.shape(1) || raw.shape(0) != dil.shape(0) || raw.shape(1) != dil.shape(1))
          throw std::invalid_argument("dilated, region and raw must be [H, W] of one shape");
        golden::SliceInput s = slice_from(raw, type, stored_bits, 1.f, 0.f, 1.f, 1.f);
        return measure_dict(golden::measure(from_np<uint8_t>(dil), from_np<uint8_t>(reg), s, connectivity));
      },
      py::arg("dilated"), py::arg("region"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("connectivity") = 8);
  // Euler number (components − holes) of a mask [H, W] from the bit-quad counts the K7 kernel uses.
  m.def(
      "measure_euler",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, int connectivity) {
        if (mask.ndim() != 2) throw std::invalid_argument("mask must be [H, W]");
        if (connectivity != 4 && connectivity != 8) throw std::invalid_argument("connectivity must be 4 or 8");
        const int h = (int)mask.shape(0), w = (int)mask.shape(1), wpr = (w + 63) / 64;
        std::vector<uint64_t> plane((size_t)h * wpr, 0ull);
        auto a = mask.unchecked<2>();
        for (int y = 0; y < h; ++y)
          for (int x = 0; x < w; ++x)
            if (a(y, x)) plane[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
        return measure::euler_plane(plane.data(), w, h, wpr, connectivity);
      },
      py::arg("mask"), py::arg("connectivity") = 8);
  m.def(
      "measure_to_json",
      [](const py::dict& rec, int w, int h, float sx, float sy, float slope, float intercept, bool apply_rescale,
         int connectivity, const py::object& intensity, const py::object& texture) {
        if (!texture.is_none()) {  // the text with the texture keys after all the others (a texture dict)
          IntensityStats st{};
          if (!intensity.is_none()) st = intensity_from(intensity.cast<py::dict>());
          return measure::to_json(measure_from(rec), nullptr, intensity.is_none() ? nullptr : &st,
                                  texture_from(texture.cast<py::dict>()), w, h, sx, sy, slope, intercept, apply_rescale,
                                  connectivity);
        }
        if (!intensity.is_none())  // the text with the intensity keys (an IntensityStats dict)
          return measure::to_json(measure_from(rec), intensity_from(intensity.cast<py::dict>()), w, h, sx, sy, slope, intercept,
                                  apply_rescale, connectivity);
        return measure::to_json(measure_from(rec), w, h, sx, sy, slope, intercept, apply_rescale, connectivity);
      },
      py::arg("record"), py::arg("w"), py::arg("h"), py::arg("spacing_x") = 1.f, py::arg("spacing_y") = 1.f,
      py::arg("slope") = 1.f, py::arg("intercept") = 0.f, py::arg("apply_rescale") = true, py::arg("connectivity") = 8,
      py::arg("intensity") = py::none(), py::arg("texture") = py::none());

  // The diameter record (nm03/measure.h SliceDiameters) of a mask [H, W] from the golden model.
  m.def(
      "golden_measure_diameters",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, int connectivity) {
        if (mask.ndim() != 2) throw std::invalid_argument("mask must be [H, W]");
        return diameters_dict(golden::measure_diameters(from_np<uint8_t>(mask), connectivity, (int)mask.shape(1), (int)mask.shape(0)));
      },
      py::arg("mask"), py::arg("connectivity") = 8);
  // The sidecar text with the diameter keys (the one function every path calls).
  m.def(
      "measure_diameters_to_json",
      [](const py::dict& rec, const py::dict& diam, int w, int h, float sx, float sy, float slope, float intercept,
         bool apply_rescale, int connectivity, const py::object& intensity, const py::object& texture) {
        if (!texture.is_none()) {
          IntensityStats st{};
          if (!intensity.is_none()) st = intensity_from(intensity.cast<py::dict>());
          const SliceDiameters sd = diameters_from(diam);
          return measure::to_json(measure_from(rec), &sd, intensity.is_none() ? nullptr : &st,
                                  texture_from(texture.cast<py::dict>()), w, h, sx, sy, slope, intercept, apply_rescale,
                                  connectivity);
        }
        if (!intensity.is_none())
          return measure::to_json(measure_from(rec), diameters_from(diam), intensity_from(intensity.cast<py::dict>()), w, h, sx,
                                  sy, slope, intercept, apply_rescale, connectivity);
        return measure::to_json(measure_from(rec), diameters_from(diam), w, h, sx, sy, slope, intercept, apply_rescale,
                                connectivity);
      },
      py::arg("record"), py::arg("diameters"), py::arg("w"), py::arg("h"), py::arg("spacing_x") = 1.f,
      py::arg("spacing_y") = 1.f, py::arg("slope") = 1.f, py::arg("intercept") = 0.f, py::arg("apply_rescale") = true,
      py::arg("connectivity") = 8, py::arg("intensity") = py::none(), py::arg("texture") = py::none());

  // ---- volume measurements (nm03/measure.h VolumeMeasure) ----------------------------------------------
  auto volume_arrays = [](const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& dil,
                          const py::array_t<uint8_t, py::array::c_style | py::array::forcecast>& reg,
                          const py::array_t<uint16_t, py::array::c_style | py::array::forcecast>& raw, const std::string& type,
                          int stored_bits) {
    if (dil.ndim() != 3 || reg.ndim() != 3 || raw.ndim() != 3)
      throw std::invalid_argument("dilated, region and raw must be [D, H, W] of one shape");
    for (int k = 0; k < 3; ++k)
      if (reg.shape(k) != dil.shape(k) || raw.shape(k) != dil.shape(k))
        throw std::invalid_argument("dilated, region and raw must be [D, H, W] of one shape");
    VolumeInput v;
    v.d = (int)dil.shape(0);
    v.h = (int)dil.shape(1);
    v.w = (int)dil.shape(2);
    VolumeMeta mt;
    mt.type = type;
    mt.stored_bits = stored_bits;
    apply_meta(mt, v);
    v.raw = from_np<uint16_t>(raw);
    return v;
  };
  m.def(
      "golden_measure_volume",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint8_t, py::array::c_style | py::array::forcecast> reg,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                      int stored_bits, int connectivity) {
        const VolumeInput v = volume_arrays(dil, reg, raw, type, stored_bits);
        const std::vector<uint8_t> dv = from_np<uint8_t>(dil), rv = from_np<uint8_t>(reg);
        VolumeMeasure r;
        {
          py::gil_scoped_release nogil;
          r = golden::measure_volume(dv, rv, v, connectivity);
        }
        return volume_measure_dict(r);
      },
      py::arg("dilated"), py::arg("region"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("connectivity") = 26);
  // The same record from the K8 kernels' word arithmetic and run union-find, run on the host one word
  // after the other (measure::volume_words): what the kernels compute, without a GPU.
  m.def(
      "measure_volume_words",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint8_t, py::array::c_style | py::array::forcecast> reg,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                      int stored_bits, int connectivity) {
        const VolumeInput v = volume_arrays(dil, reg, raw, type, stored_bits);
        const std::vector<uint64_t> dw = pack_volume(dil), rw = pack_volume(reg);
        return volume_measure_dict(measure::volume_words(dw.data(), rw.data(), v.raw.data(), (size_t)v.w * v.h, v.w, v.h, v.d,
                                                         (v.w + 63) / 64, (uint8_t)v.type, (uint8_t)v.stored_bits, connectivity));
      },
      py::arg("dilated"), py::arg("region"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("connectivity") = 26);
  // Words of K8's labelling scratch, (w + 1)·h·d + 1; 0 for a volume too large to measure (≥ 2^32).
  m.def("volume_measure_scratch_words", [](int w, int h, int d) { return volume_measure_scratch_words(w, h, d); });
  m.def(
      "volume_measure_to_json",
      [](const py::dict& rec, int w, int h, int d, double sx, double sy, double sz, const std::string& source, float slope,
         float intercept, bool apply_rescale, int connectivity, const py::object& lesions, int lesions_max,
         const py::object& intensity, const py::object& texture, const py::object& diameters, const py::object& spacing_um,
         const py::object& thickness) {
        // `thickness` (a thickness dict): the thickness keys after the global keys, at `spacing_um` or the
        // quantised spacings.
        auto with_thickness = [&](std::string text) {
          if (thickness.is_none()) return text;
          uint32_t um[3];
          if (spacing_um.is_none()) measure::volume_spacing_um((double)(float)sx, (double)(float)sy, sz, um);
          else spacing_um_from(spacing_um.cast<std::vector<int64_t>>(), um);
          return measure::insert_thickness_keys(std::move(text), volume_thickness_from(thickness.cast<py::dict>()), um);
        };
        // `diameters` (a list of diameter dicts, one per lesion): the text below with the diameter keys, at
        // `spacing_um` (ux, uy, uz) or, when that is None, the quantised spacings.
        auto with_diameters = [&](std::string text) {
          text = with_thickness(std::move(text));
          if (diameters.is_none()) return text;
          if (lesions.is_none()) throw std::invalid_argument("diameters need lesions");
          std::vector<VolumeLesionDiameters> ds;
          for (const py::handle& x : diameters.cast<py::list>()) ds.push_back(volume_diameters_from(x.cast<py::dict>()));
          if (ds.size() != py::len(lesions)) throw std::invalid_argument("one diameter dict per lesion");
          uint32_t um[3];
          if (spacing_um.is_none()) measure::volume_spacing_um((double)(float)sx, (double)(float)sy, sz, um);
          else spacing_um_from(spacing_um.cast<std::vector<int64_t>>(), um);
          return measure::insert_diameter_keys(std::move(text), ds.data(), (int)ds.size(), um);
        };
        // Pixel spacings pass through float, as VolumeInput holds them.
        if (!texture.is_none()) {  // the text with the texture keys after the global keys (a texture dict)
          IntensityStats st{};
          if (!intensity.is_none()) st = intensity_from(intensity.cast<py::dict>());
          std::vector<VolumeLesion> ls;
          if (!lesions.is_none()) {
            for (const py::handle& l : lesions.cast<py::list>()) ls.push_back(volume_lesion_from(l.cast<py::dict>()));
            check_max_lesions(lesions_max);
            if (ls.size() > (size_t)lesions_max) throw std::invalid_argument("more lesions than lesions_max");
          }
          return with_diameters(measure::volume_to_json(volume_measure_from(rec), intensity.is_none() ? nullptr : &st, ls.data(), (int)ls.size(),
                                         lesions.is_none() ? 0 : lesions_max, texture_from(texture.cast<py::dict>()), w, h, d,
                                         (double)(float)sx, (double)(float)sy, sz, source, slope, intercept, apply_rescale,
                                         connectivity));
        }
        if (lesions.is_none()) {
          if (!intensity.is_none())  // the text with the intensity keys (an IntensityStats dict)
            return with_diameters(measure::volume_to_json(volume_measure_from(rec), intensity_from(intensity.cast<py::dict>()), w, h, d,
                                           (double)(float)sx, (double)(float)sy, sz, source, slope, intercept, apply_rescale,
                                           connectivity));
          return with_diameters(measure::volume_to_json(volume_measure_from(rec), w, h, d, (double)(float)sx, (double)(float)sy, sz, source,
                                         slope, intercept, apply_rescale, connectivity));
        }
        // With `lesions` (a list of lesion dicts, as many as are reported): the text with the lesion keys.
        std::vector<VolumeLesion> ls;
        for (const py::handle& l : lesions.cast<py::list>()) ls.push_back(volume_lesion_from(l.cast<py::dict>()));
        check_max_lesions(lesions_max);
        if (ls.size() > (size_t)lesions_max) throw std::invalid_argument("more lesions than lesions_max");
        if (!intensity.is_none())
          return with_diameters(measure::volume_to_json(volume_measure_from(rec), intensity_from(intensity.cast<py::dict>()), ls.data(),
                                         (int)ls.size(), lesions_max, w, h, d, (double)(float)sx, (double)(float)sy, sz, source,
                                         slope, intercept, apply_rescale, connectivity));
        return with_diameters(measure::volume_to_json(volume_measure_from(rec), ls.data(), (int)ls.size(), lesions_max, w, h, d,
                                       (double)(float)sx, (double)(float)sy, sz, source, slope, intercept, apply_rescale,
                                       connectivity));
      },
      py::arg("record"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing_x") = 1.0, py::arg("spacing_y") = 1.0,
      py::arg("spacing_z") = 1.0, py::arg("spacing_z_source") = "default", py::arg("slope") = 1.f,
      py::arg("intercept") = 0.f, py::arg("apply_rescale") = true, py::arg("connectivity") = 26,
      py::arg("lesions") = py::none(), py::arg("lesions_max") = 0, py::arg("intensity") = py::none(),
      py::arg("texture") = py::none(), py::arg("diameters") = py::none(), py::arg("spacing_um") = py::none(),
      py::arg("thickness") = py::none());
  // The N largest components of a volume mask (nm03/measure.h VolumeLesion) by the golden model (flood
  // fill per component) → list of dicts of the records' integers, largest first.
  m.def(
      "golden_measure_volume_lesions",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int max_lesions,
                      const std::string& type, int stored_bits, int connectivity) {
        check_max_lesions(max_lesions);
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        const std::vector<uint8_t> dv = from_np<uint8_t>(dil);
        std::vector<VolumeLesion> r;
        {
          py::gil_scoped_release nogil;
          r = golden::measure_volume_lesions(dv, v, connectivity, max_lesions);
        }
        return volume_lesion_list(r.data(), r.size());
      },
      py::arg("dilated"), py::arg("raw"), py::arg("max_lesions"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("connectivity") = 26);
  // The same records from the K10 kernels' per-word lesion logic on K8's run union-find, run on the host
  // one word after the other (measure::volume_lesions_words).
  m.def(
      "volume_lesions_words",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int max_lesions,
                      const std::string& type, int stored_bits, int connectivity) {
        check_max_lesions(max_lesions);
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        const std::vector<uint64_t> dw = pack_volume(dil);
        std::vector<VolumeLesion> r((size_t)max_lesions);
        const int n = measure::volume_lesions_words(dw.data(), v.raw.data(), (size_t)v.w * v.h, v.w, v.h, v.d, (v.w + 63) / 64,
                                                    (uint8_t)v.type, (uint8_t)v.stored_bits, connectivity, max_lesions, r.data());
        return volume_lesion_list(r.data(), (size_t)n);
      },
      py::arg("dilated"), py::arg("raw"), py::arg("max_lesions"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("connectivity") = 26);
  // The lengths of the same lesions (nm03/measure.h VolumeLesionDiameters) by the golden model: flood fill,
  // then plain loops over the pairs of open-face voxels → list of dicts of the records' integers.
  m.def(
      "golden_measure_volume_diameters",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil, int max_lesions,
         const std::vector<int64_t>& spacing_um, int connectivity) {
        check_max_lesions(max_lesions);
        if (dil.ndim() != 3) throw std::invalid_argument("dilated must be [D, H, W]");
        uint32_t um[3];
        spacing_um_from(spacing_um, um);
        const int d = (int)dil.shape(0), h = (int)dil.shape(1), w = (int)dil.shape(2);
        const std::vector<uint8_t> dv = from_np<uint8_t>(dil);
        std::vector<VolumeLesionDiameters> r;
        {
          py::gil_scoped_release nogil;
          r = golden::measure_volume_diameters(dv, w, h, d, connectivity, max_lesions, um);
        }
        return volume_diameters_list(r.data(), r.size());
      },
      py::arg("dilated"), py::arg("max_lesions"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000},
      py::arg("connectivity") = 26);
  // The same records from the K13 kernels' logic run on the host (measure::volume_diameters_words);
  // with_skipped = true → (records, tile pairs the bound skipped).
  m.def(
      "volume_diameters_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil, int max_lesions,
         const std::vector<int64_t>& spacing_um, int connectivity, bool brute_force, bool with_skipped) -> py::object {
        check_max_lesions(max_lesions);
        if (dil.ndim() != 3) throw std::invalid_argument("dilated must be [D, H, W]");
        uint32_t um[3];
        spacing_um_from(spacing_um, um);
        const int d = (int)dil.shape(0), h = (int)dil.shape(1), w = (int)dil.shape(2);
        if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
        const std::vector<uint64_t> dw = pack_volume(dil);
        std::vector<VolumeLesionDiameters> r((size_t)max_lesions);
        uint64_t skipped = 0;
        int n = 0;
        {
          py::gil_scoped_release nogil;
          n = measure::volume_diameters_words(dw.data(), w, h, d, (w + 63) / 64, connectivity, max_lesions, um, brute_force,
                                              r.data(), &skipped);
        }
        py::list out = volume_diameters_list(r.data(), (size_t)n);
        if (with_skipped) return py::make_tuple(out, skipped);
        return out;
      },
      py::arg("dilated"), py::arg("max_lesions"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000},
      py::arg("connectivity") = 26, py::arg("brute_force") = false, py::arg("with_skipped") = false);
  // The spacing in integer micrometres the diameters are maximised in: max(1, llround(mm · 1000)) per axis.
  m.def("volume_spacing_um", [](double sx, double sy, double sz) {
    uint32_t um[3];
    measure::volume_spacing_um(sx, sy, sz, um);
    return py::make_tuple(um[0], um[1], um[2]);
  }, py::arg("spacing_x"), py::arg("spacing_y"), py::arg("spacing_z"));
  m.attr("MAX_VOLUME_LESIONS") = kMaxVolumeLesions;

  // ---- intensity statistics (nm03/measure.h IntensityStats) ----------------------------------------------
  // The nearest rank of percentile p among n samples (nm03/intensity_core.h) and the raw standard
  // deviation of a record (the exact 128-bit radicand), as the sidecar text uses them.
  m.def("intensity_rank", [](uint32_t p, uint64_t n) { return icore::percentile_rank(p, n); });
  m.def("intensity_std", [](const py::dict& rec, int64_t raw_sum) { return measure::intensity_std(intensity_from(rec), raw_sum); });
  // The golden model (collect, sort, index) on a mask [H, W] and its 16-bit samples.
  m.def(
      "golden_measure_intensity",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
         py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type, int stored_bits) {
        if (dil.ndim() != 2 || raw.ndim() != 2 || raw.shape(0) != dil.shape(0) || raw.shape(1) != dil.shape(1))
          throw std::invalid_argument("dilated and raw must be [H, W] of one shape");
        const golden::SliceInput s = slice_from(raw, type, stored_bits, 1.f, 0.f, 1.f, 1.f);
        return intensity_dict(golden::measure_intensity(from_np<uint8_t>(dil), s));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16);
  m.def(
      "golden_measure_volume_intensity",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                      int stored_bits) {
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        return intensity_dict(golden::measure_intensity(from_np<uint8_t>(dil), v));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16);
  // The same records from the K11 kernels' two-pass radix select run on the host over bit planes
  // (measure::intensity_words). `stray_bits`: also set every storage bit past the width, which must not count.
  m.def(
      "intensity_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
         py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type, int stored_bits,
         bool stray_bits) {
        if (dil.ndim() != 2 || raw.ndim() != 2 || raw.shape(0) != dil.shape(0) || raw.shape(1) != dil.shape(1))
          throw std::invalid_argument("dilated and raw must be [H, W] of one shape");
        const golden::SliceInput s = slice_from(raw, type, stored_bits, 1.f, 0.f, 1.f, 1.f);
        const int wpr = (s.w + 63) / 64;
        std::vector<uint64_t> plane((size_t)s.h * wpr, 0ull);
        auto a = dil.unchecked<2>();
        for (int y = 0; y < s.h; ++y) {
          for (int x = 0; x < s.w; ++x)
            if (a(y, x)) plane[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
          if (stray_bits) plane[(size_t)y * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, s.w);
        }
        return intensity_dict(measure::intensity_words(plane.data(), s.raw.data(), (size_t)s.w * s.h, s.w, s.h, 1, wpr,
                                                       (uint8_t)s.type, (uint8_t)s.stored_bits));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("stray_bits") = false);
  m.def(
      "volume_intensity_words",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
                      int stored_bits) {
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        const std::vector<uint64_t> dw = pack_volume(dil);
        return intensity_dict(measure::intensity_words(dw.data(), v.raw.data(), (size_t)v.w * v.h, v.w, v.h, v.d,
                                                       (v.w + 63) / 64, (uint8_t)v.type, (uint8_t)v.stored_bits));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16);

  // ---- texture (nm03/texture_core.h, nm03/measure.h TextureGlcm) -----------------------------------------
  m.def("texture_level", [](uint32_t key, uint32_t lo, uint32_t hi, uint32_t levels) { return tcore::level(key, lo, hi, levels); });
  // Everything the sidecar derives from a co-occurrence matrix [levels, levels] (measure::glcm_features):
  // the 7 integers and the 16 doubles under their sidecar keys, None where the text says null.
  m.def("glcm_features", [](py::array_t<uint32_t, py::array::c_style | py::array::forcecast> c) {
    if (c.ndim() != 2 || c.shape(0) != c.shape(1) || c.shape(0) < 2 || c.shape(0) > 64)
      throw std::invalid_argument("glcm must be [levels, levels] with 2 <= levels <= 64");
    return glcm_features_dict(measure::glcm_features(c.data(), (int)c.shape(0)));
  });
  m.def("texture_keys", [](py::array_t<uint32_t, py::array::c_style | py::array::forcecast> c) {
    if (c.ndim() != 2 || c.shape(0) != c.shape(1) || c.shape(0) < 2 || c.shape(0) > 64)
      throw std::invalid_argument("glcm must be [levels, levels] with 2 <= levels <= 64");
    return measure::texture_keys(c.data(), (int)c.shape(0));
  });
  // The golden model (a loop over voxels and directions) on a mask [H, W] and its 16-bit samples.
  m.def(
      "golden_measure_texture",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
         py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int levels, const std::string& type,
         int stored_bits) {
        if (dil.ndim() != 2 || raw.ndim() != 2 || raw.shape(0) != dil.shape(0) || raw.shape(1) != dil.shape(1))
          throw std::invalid_argument("dilated and raw must be [H, W] of one shape");
        const golden::SliceInput s = slice_from(raw, type, stored_bits, 1.f, 0.f, 1.f, 1.f);
        return texture_dict(golden::measure_texture(from_np<uint8_t>(dil), s, levels));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("levels") = 32, py::arg("type") = "u16", py::arg("stored_bits") = 16);
  m.def(
      "golden_measure_volume_texture",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int levels, const std::string& type,
                      int stored_bits) {
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        return texture_dict(golden::measure_texture(from_np<uint8_t>(dil), v, levels));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("levels") = 32, py::arg("type") = "u16", py::arg("stored_bits") = 16);
  // The same records from the K12 kernels' per-word pair logic run on the host over bit planes
  // (measure::texture_words). `stray_bits`: also set every storage bit past the width, which must not pair.
  m.def(
      "texture_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
         py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int levels, const std::string& type,
         int stored_bits, bool stray_bits) {
        if (dil.ndim() != 2 || raw.ndim() != 2 || raw.shape(0) != dil.shape(0) || raw.shape(1) != dil.shape(1))
          throw std::invalid_argument("dilated and raw must be [H, W] of one shape");
        const golden::SliceInput s = slice_from(raw, type, stored_bits, 1.f, 0.f, 1.f, 1.f);
        const int wpr = (s.w + 63) / 64;
        std::vector<uint64_t> plane((size_t)s.h * wpr, 0ull);
        auto a = dil.unchecked<2>();
        for (int y = 0; y < s.h; ++y) {
          for (int x = 0; x < s.w; ++x)
            if (a(y, x)) plane[(size_t)y * wpr + (x >> 6)] |= 1ull << (x & 63);
          if (stray_bits) plane[(size_t)y * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, s.w);
        }
        return texture_dict(measure::texture_words(plane.data(), s.raw.data(), (size_t)s.w * s.h, s.w, s.h, 1, wpr,
                                                   (uint8_t)s.type, (uint8_t)s.stored_bits, levels));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("levels") = 32, py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("stray_bits") = false);
  m.def(
      "volume_texture_words",
      [volume_arrays](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dil,
                      py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, int levels, const std::string& type,
                      int stored_bits) {
        const VolumeInput v = volume_arrays(dil, dil, raw, type, stored_bits);
        const std::vector<uint64_t> dw = pack_volume(dil);
        return texture_dict(measure::texture_words(dw.data(), v.raw.data(), (size_t)v.w * v.h, v.w, v.h, v.d, (v.w + 63) / 64,
                                                   (uint8_t)v.type, (uint8_t)v.stored_bits, levels));
      },
      py::arg("dilated"), py::arg("raw"), py::arg("levels") = 32, py::arg("type") = "u16", py::arg("stored_bits") = 16);

  // ---- JPEG --------------------------------------------------------------------------------------
  m.def("jpeg_encode_gray420", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> g, int quality) {
    const int h = (int)g.shape(0), w = (int)g.shape(1);
    auto b = jpeg::encode_gray(g.data(), w, h, w, quality);
    return py::bytes((const char*)b.data(), b.size());
  }, py::arg("gray"), py::arg("quality") = 75);
  // sampling: jpeg::Sampling (0 YCbCr 4:2:0, 1 YCbCr 4:4:4, 2 one gray component).
  m.def("jpeg_encode_gray", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> g, int quality,
                               int sampling) {
    if (sampling < 0 || sampling > 2) throw std::invalid_argument("sampling must be 0, 1 or 2");
    const int h = (int)g.shape(0), w = (int)g.shape(1);
    auto b = jpeg::encode_gray(g.data(), w, h, w, quality, (jpeg::Sampling)sampling);
    return py::bytes((const char*)b.data(), b.size());
  }, py::arg("gray"), py::arg("quality") = 75, py::arg("sampling") = 0);
  // Interleaved RGB [H, W, 3] → complete colour JFIF file (golden encoder; sampling 0 or 1).
  m.def("jpeg_encode_rgb", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> rgb, int quality,
                              int sampling) {
    if (rgb.ndim() != 3 || rgb.shape(2) != 3) throw std::invalid_argument("rgb must be [H, W, 3] uint8");
    if (sampling != 0 && sampling != 1) throw std::invalid_argument("a colour image needs sampling 0 (4:2:0) or 1 (4:4:4)");
    const int h = (int)rgb.shape(0), w = (int)rgb.shape(1);
    auto b = jpeg::encode_rgb(rgb.data(), w, h, 3 * w, quality, (jpeg::Sampling)sampling);
    return py::bytes((const char*)b.data(), b.size());
  }, py::arg("rgb"), py::arg("quality") = 75, py::arg("sampling") = 0);
  m.def("jpeg_header", [](int w, int h, int quality, int sampling) {
    if (sampling < 0 || sampling > 2) throw std::invalid_argument("sampling must be 0, 1 or 2");
    auto b = jpeg::make_header(w, h, jpeg::make_tables(quality), (jpeg::Sampling)sampling);
    return py::bytes((const char*)b.data(), b.size());
  }, py::arg("w"), py::arg("h"), py::arg("quality") = 75, py::arg("sampling") = 0);
  m.def("jpeg_quant_tables", [](int quality) {
    auto t = jpeg::make_tables(quality);
    return py::make_tuple(std::vector<int>(t.qluma, t.qluma + 64), std::vector<int>(t.qchroma, t.qchroma + 64));
  });

  // ---- engine --------------------------------------------------------------------------------------
  // A work list converted once to its native form (the cohort plan), reusable across runs and
  // shared with the engine while a submitted run is in flight.
  struct WorkList {
    std::shared_ptr<std::vector<WorkItem>> items = std::make_shared<std::vector<WorkItem>>();
  };
  py::class_<WorkList>(m, "WorkList")
      .def(py::init([](const std::vector<std::pair<std::string, std::string>>& items) {
        WorkList w;
        w.items->reserve(items.size());
        for (auto& p : items) w.items->push_back({p.first, p.second});
        return w;
      }))
      .def("__len__", [](const WorkList& w) { return w.items->size(); })
      .def("items", [](const WorkList& w) {
        std::vector<std::pair<std::string, std::string>> v;
        v.reserve(w.items->size());
        for (auto& it : *w.items) v.push_back({it.path, it.out_dir});
        return v;
      })
      // A reference run's set-up in one native call (main_sequential.cpp:93-168, 32-47): discover
      // the PGBM-* patients under data_root's cohort directory, per patient wipe (through `reaper`:
      // rename aside + background deletion) or create <out_root>/<pid>, list its first series in
      // reference order, and build the work list.
      .def_static(
          "discover",
          [](const std::string& data_root, const std::string& out_root, cohort::OutputReaper* reaper) {
            py::gil_scoped_release nogil;
            WorkList w;
            const std::string base = cohort::cohort_dir(data_root);
            for (const auto& pid : cohort::find_patient_dirs(base)) {
              const std::string out = out_root + "/" + pid;
              if (reaper)
                reaper->wipe(out);
              else
                cohort::make_dirs(out);
              cohort::Series s = cohort::list_patient_series(base, pid);
              for (auto& f : s.files) w.items->push_back({std::move(f), out});
            }
            return w;
          },
          py::arg("data_root"), py::arg("out_root"), py::arg("reaper") = nullptr);
  struct Ticket {
    RunTicket t;
  };
  py::class_<Ticket>(m, "RunTicket");
  auto times_dict = [](const StageTimes& t) {
    py::dict td;
    td["load_s"] = t.load_s;
    td["h2d_s"] = t.h2d_s;
    td["kernels_s"] = t.kernels_s;
    td["write_s"] = t.write_s;
    td["load_cpu_s"] = t.load_cpu_s;
    td["write_cpu_s"] = t.write_cpu_s;
    td["slot_cpu_s"] = t.slot_cpu_s;
    td["wall_s"] = t.wall_s;
    td["batches"] = t.batches;
    td["slices_ok"] = t.slices_ok;
    td["slices_failed"] = t.slices_failed;
    td["bytes_in"] = t.bytes_in;
    td["bytes_out"] = t.bytes_out;
    td["jpeg_fallbacks"] = t.jpeg_fallbacks;
    return td;
  };
  auto compact = [times_dict](const std::vector<SliceStatus>& st, const StageTimes& t) {
    py::array_t<int32_t> codes((py::ssize_t)st.size());
    auto c = codes.mutable_unchecked<1>();
    py::dict msgs;
    for (size_t i = 0; i < st.size(); ++i) {
      c((py::ssize_t)i) = st[i].code;
      if (st[i].code != kSliceOk) msgs[py::int_(i)] = st[i].message;
    }
    return py::make_tuple(codes, msgs, times_dict(t));
  };
  py::class_<Engine>(m, "Engine")
      .def(py::init<const EngineConfig&>())
      .def(
          "run",
          [times_dict](Engine& e, const std::vector<std::pair<std::string, std::string>>& items) {
            std::vector<WorkItem> wi;
            for (auto& p : items) wi.push_back({p.first, p.second});
            StageTimes t;
            std::vector<SliceStatus> st;
            {
              py::gil_scoped_release nogil;
              st = e.run(wi, &t);
            }
            std::vector<std::pair<int, std::string>> out;
            for (auto& s : st) out.push_back({s.code, s.message});
            return py::make_tuple(out, times_dict(t));
          })
      .def(
          "run_list",
          // Compact form for hot loops: (codes int32[n], {index: message} for non-OK slices, times).
          [compact](Engine& e, const WorkList& wl, int batch_cap) {
            StageTimes t;
            std::vector<SliceStatus> st;
            {
              py::gil_scoped_release nogil;
              st = e.run(*wl.items, &t, {}, batch_cap);
            }
            return compact(st, t);
          },
          py::arg("work"), py::arg("batch_cap") = 0)
      .def(
          "submit",
          // Queue a run and return at once (Engine::submit); the next run can be submitted before
          // this one finished — the engine pipelines across them.
          [](Engine& e, const WorkList& wl, int batch_cap) {
            py::gil_scoped_release nogil;
            return Ticket{e.submit(wl.items, {}, batch_cap)};
          },
          py::arg("work"), py::arg("batch_cap") = 0)
      .def(
          "wait",
          // Result of a submitted run, in run_list's compact form.
          [compact](Engine& e, const Ticket& t) {
            StageTimes tm;
            std::vector<SliceStatus> st;
            {
              py::gil_scoped_release nogil;
              st = e.wait(t.t, &tm);
            }
            return compact(st, tm);
          })
      .def("run_single",
           [](Engine& e, py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw, const std::string& type,
              int stored_bits, float slope, float intercept, float sx, float sy) {
             golden::SliceInput s = slice_from(raw, type, stored_bits, slope, intercept, sx, sy);
             SingleResult r;
             {
               py::gil_scoped_release nogil;
               r = e.run_single(s);
             }
             py::dict d;
             d["median_keys"] = to_np<uint16_t>(r.median_keys, {r.h, r.w});
             d["sharpened"] = to_np<float>(r.sharpened, {r.h, r.w});
             d["band"] = mask2d(r.band, r.h, r.w);
             d["region"] = mask2d(r.region, r.h, r.w);
             d["eroded"] = mask2d(r.eroded, r.h, r.w);
             d["dilated"] = mask2d(r.dilated, r.h, r.w);
             d["border_region"] = mask2d(r.border_region, r.h, r.w);
             d["border_eroded"] = mask2d(r.border_eroded, r.h, r.w);
             d["border_dilated"] = mask2d(r.border_dilated, r.h, r.w);
             py::list cv, jp;
             const int cw = e.config().render.out_width, ch = e.config().render.out_height;
             for (auto& c : r.canvases) cv.append(to_np<uint8_t>(c, {ch, cw}));
             for (auto& j : r.jpegs) jp.append(py::bytes((const char*)j.data(), j.size()));
             d["canvases"] = cv;
             d["jpegs"] = jp;
             if (e.config().render.overlay) {
               d["overlay"] = to_np<uint8_t>(r.overlay, {ch, cw, 3});
               d["jpeg_overlay"] = py::bytes((const char*)r.jpeg_overlay.data(), r.jpeg_overlay.size());
             }
             if (e.config().pipe.measure) {
               d["measure"] = measure_dict(r.measure);
               d["measure_json"] = r.measure_json;
               if (e.config().pipe.measure_diameters) d["diameters"] = diameters_dict(r.diameters);
               if (e.config().pipe.measure_intensity) d["intensity"] = intensity_dict(r.intensity);
               if (e.config().pipe.measure_texture) d["texture"] = texture_dict(r.texture);
             }
             return d;
           },
           py::arg("raw"), py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("slope") = 1.f,
           py::arg("intercept") = 0.f, py::arg("spacing_x") = 1.f, py::arg("spacing_y") = 1.f);
  m.def("device_count", &device_count);
  // CPU sampling profiler (cpu_sampler.h; bench.py --cpu-profile, tools/cpu_profile.py).
  m.def("cpu_profile_start", &prof::sampler_start, py::arg("period_us") = 250, py::arg("max_samples") = 1 << 20,
        py::arg("depth") = 24);
  m.def("cpu_profile_stop", &prof::sampler_stop, py::arg("path"), py::call_guard<py::gil_scoped_release>());

  // ---- 3D ---------------------------------------------------------------------------------------------
  m.def(
      "run_volume",
      [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> vol, const PipelineParams& p, int connectivity,
         int dilation, const std::vector<std::tuple<int, int, int>>& seeds, int device) {
        return volume_call(vol, p, connectivity, dilation, seeds, [device](const VolumeInput& v, const VolumeParams& vp) {
          return run_volume(v, vp, device, true);
        });
      },
      py::arg("volume"), py::arg("params") = PipelineParams(), py::arg("connectivity") = 6, py::arg("dilation") = 7,
      py::arg("seeds") = std::vector<std::tuple<int, int, int>>{}, py::arg("device") = 0);
  // Persistent runner: device buffers, stream, events and pinned staging are kept across volumes
  // (0.94 ms per 256^3 volume vs ~8.7 ms for the one-shot run_volume).
  py::class_<VolumeRunner>(m, "VolumeRunner")
      .def(py::init<int>(), py::arg("device") = 0)
      .def(
          "run",
          [](VolumeRunner& self, py::array_t<uint16_t, py::array::c_style | py::array::forcecast> vol,
             const PipelineParams& p, int connectivity, int dilation,
             const std::vector<std::tuple<int, int, int>>& seeds, bool measure, int measure_connectivity,
             const std::vector<double>& spacing, const std::string& spacing_z_source, const std::string& type,
             int stored_bits, float slope, float intercept, int measure_lesions, bool measure_intensity, bool measure_texture,
             int texture_levels, bool measure_diameters, int64_t dilate_um, bool measure_thickness, const py::object& compare_to,
             const std::string& compare_reference, int compare_lesions) {
            VolumeMeta mt;
            compare_to_from(compare_to, compare_reference, mt);
            mt.compare_lesions = compare_lesions;
            mt.measure_diameters = measure_diameters;
            mt.dilate_um = dilate_um;
            mt.measure_thickness = measure_thickness;
            mt.measure_lesions = measure_lesions;
            mt.measure_intensity = measure_intensity;
            mt.measure_texture = measure_texture;
            mt.texture_levels = texture_levels;
            mt.type = type;
            mt.stored_bits = stored_bits;
            mt.slope = slope;
            mt.intercept = intercept;
            mt.spacing = spacing;
            mt.spacing_z_source = spacing_z_source;
            mt.measure = measure;
            mt.measure_connectivity = measure_connectivity;
            return volume_call(vol, p, connectivity, dilation, seeds,
                               [&self](const VolumeInput& v, const VolumeParams& vp) { return self.run(v, vp, true); }, &mt);
          },
          py::arg("volume"), py::arg("params") = PipelineParams(), py::arg("connectivity") = 6,
          py::arg("dilation") = 7, py::arg("seeds") = std::vector<std::tuple<int, int, int>>{},
          py::arg("measure") = false, py::arg("measure_connectivity") = 26,
          py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0}, py::arg("spacing_z_source") = "default",
          py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("slope") = 1.f, py::arg("intercept") = 0.f,
          py::arg("measure_lesions") = 0, py::arg("measure_intensity") = false, py::arg("measure_texture") = false,
          py::arg("texture_levels") = 32, py::arg("measure_diameters") = false, py::arg("dilate_um") = -1,
          py::arg("measure_thickness") = false, py::arg("compare_to") = py::none(), py::arg("compare_reference") = "",
          py::arg("compare_lesions") = 0)
      .def(
          "export_views",
          // After run() on a volume of this shape: the views of nm03/volume_views.h from the volume still on
          // the device (K14, K3, K4). Returns the views_dict keys plus views_json (the sidecar text),
          // views_jpeg (file name → bytes), k14_s and render_s.
          [](VolumeRunner& self, int w, int h, int d, const PipelineParams& p, const RenderParams& rp, const py::object& at,
             const std::vector<double>& spacing, const std::string& type, int stored_bits, float slope, float intercept) {
            VolumeMeta mt;
            mt.type = type;
            mt.stored_bits = stored_bits;
            mt.slope = slope;
            mt.intercept = intercept;
            mt.spacing = spacing;
            VolumeInput v;
            v.w = w, v.h = h, v.d = d;
            apply_meta(mt, v);
            VolumeParams vp;
            vp.pipe = p;
            const ViewsAt a = views_at_from(at);
            VolumeViewsExport x;
            {
              py::gil_scoped_release nogil;
              x = self.export_views(v, vp, rp, a, true);
            }
            py::dict out = views_dict(x.views);
            out["views_json"] = views::to_json(x.views, v.spacing_x, v.spacing_y, v.spacing_z);
            out["views_jpeg"] = view_files_dict(x.files);
            out["k14_s"] = x.k14_s;
            out["render_s"] = x.render_s;
            return out;
          },
          py::arg("w"), py::arg("h"), py::arg("d"), py::arg("params") = PipelineParams(), py::arg("render") = RenderParams(),
          py::arg("at") = py::str("mask"), py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0}, py::arg("type") = "u16",
          py::arg("stored_bits") = 16, py::arg("slope") = 1.f, py::arg("intercept") = 0.f)
      .def(
          "export_mesh",
          // After run() on a volume of this shape: the surface mesh of nm03/volume_mesh.h from the dilated bit
          // planes still on the device (K15). Returns the mesh dict; a mesh above max_bytes raises RuntimeError.
          [](VolumeRunner& self, int w, int h, int d, const std::string& placement, const std::vector<double>& spacing,
             uint64_t max_bytes, int scan_block) {
            VolumeMeta mt;
            mt.spacing = spacing;
            VolumeInput v;
            v.w = w, v.h = h, v.d = d;
            apply_meta(mt, v);
            const int pl = mesh_placement_from(placement);
            VolumeMesh m;
            {
              py::gil_scoped_release nogil;
              m = self.export_mesh(v, VolumeParams(), pl, max_bytes, scan_block);
            }
            return mesh_dict(m);
          },
          py::arg("w"), py::arg("h"), py::arg("d"), py::arg("placement") = "corner",
          py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0}, py::arg("max_bytes") = mesh::kDefaultMaxMb << 20,
          py::arg("scan_block") = 0)
      .def(
          "run_slab",
          // One rank's z-slab (planes [z0, z0 + slab depth) of a `depth`-deep volume) through the
          // distributed 3D pipeline over `comm` (collective; volume_slabs.h). Seeds in volume
          // coordinates. Returns the slab's masks plus rounds / exchanged bytes.
          [](VolumeRunner& self, Comm& comm, py::array_t<uint16_t, py::array::c_style | py::array::forcecast> slab,
             int z0, int depth, const PipelineParams& p, int connectivity, int dilation,
             const std::vector<std::tuple<int, int, int>>& seeds, bool measure, int measure_lesions, bool measure_intensity,
             bool measure_texture, bool measure_diameters, int64_t dilate_um, bool measure_thickness, const py::object& compare_to,
             int compare_lesions) {
            SlabStats st;
            VolumeMeta mt;
            compare_to_from(compare_to, "", mt);  // refused by run_slab
            mt.compare_lesions = compare_lesions;  // alike
            mt.measure_diameters = measure_diameters;
            mt.dilate_um = dilate_um;  // refused by run_slab, as the measurements are
            mt.measure_thickness = measure_thickness;
            mt.measure = measure;  // refused by run_slab (std::invalid_argument) before anything is launched
            mt.measure_lesions = measure_lesions;  // alike
            mt.measure_intensity = measure_intensity;
            mt.measure_texture = measure_texture;
            py::dict d = volume_call(slab, p, connectivity, dilation, seeds,
                                     [&](const VolumeInput& v, const VolumeParams& vp) {
                                       return self.run_slab(comm, v, z0, depth, vp, true, &st);
                                     }, &mt);
            d["rounds"] = st.rounds;
            d["exchanged_bytes"] = st.exchanged_bytes;
            return d;
          },
          py::arg("comm"), py::arg("slab"), py::arg("z0"), py::arg("depth"), py::arg("params") = PipelineParams(),
          py::arg("connectivity") = 6, py::arg("dilation") = 7,
          py::arg("seeds") = std::vector<std::tuple<int, int, int>>{}, py::arg("measure") = false,
          py::arg("measure_lesions") = 0, py::arg("measure_intensity") = false, py::arg("measure_texture") = false,
          py::arg("measure_diameters") = false, py::arg("dilate_um") = -1, py::arg("measure_thickness") = false,
          py::arg("compare_to") = py::none(), py::arg("compare_lesions") = 0);

  // One-process rehearsal of the z-slab decomposition: `nranks` threads, each with its own
  // VolumeRunner (stream) on `device`, talking over loopback comms — the device-resident exchange
  // (Comm::sendrecv_device staged through pinned memory here) without the inter-process GPU
  // time-slicing that several rank processes on one GPU add. Runs `repeats` timed splits after one
  // warm-up; returns the wall times (max over ranks per split, seconds), the last split's rounds /
  // exchanged bytes per rank and its gathered masks.
  m.def(
      "run_volume_slabs_threads",
      [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> vol, int nranks, const PipelineParams& p,
         int connectivity, int dilation, int device, int repeats) {
        if (vol.ndim() != 3) throw std::invalid_argument("volume must be (depth, height, width)");
        const int D = (int)vol.shape(0), H = (int)vol.shape(1), W = (int)vol.shape(2);
        if (nranks < 1 || nranks > D) throw std::invalid_argument("1 <= nranks <= depth");
        const std::vector<uint16_t> raw = from_np<uint16_t>(vol);
        std::vector<VolumeInput> slabs((size_t)nranks);
        for (int r = 0; r < nranks; ++r) {
          const auto [z0, z1] = slab_bounds(D, r, nranks);
          VolumeInput& v = slabs[(size_t)r];
          v.w = W;
          v.h = H;
          v.d = z1 - z0;
          v.raw.assign(raw.begin() + (size_t)z0 * W * H, raw.begin() + (size_t)z1 * W * H);
        }
        VolumeParams vp;
        vp.pipe = p;
        vp.connectivity = connectivity;
        vp.dilation_size = dilation;
        std::vector<double> walls;
        std::vector<VolumeResult> res((size_t)nranks);
        std::vector<SlabStats> st((size_t)nranks);
        {
          py::gil_scoped_release nogil;
          std::vector<std::unique_ptr<VolumeRunner>> runners;
          for (int r = 0; r < nranks; ++r) runners.push_back(std::make_unique<VolumeRunner>(device));
          auto group = make_loopback_group(nranks);
          for (int rep = 0; rep <= repeats; ++rep) {
            const bool last = rep == repeats;
            std::vector<double> t((size_t)nranks);
            std::vector<std::string> err((size_t)nranks);
            std::vector<std::thread> th;
            for (int r = 0; r < nranks; ++r)
              th.emplace_back([&, r] {
                try {
                  const auto zz = slab_bounds(D, r, nranks);
                  group[(size_t)r]->barrier();
                  const auto t0 = std::chrono::steady_clock::now();
                  res[(size_t)r] = runners[(size_t)r]->run_slab(*group[(size_t)r], slabs[(size_t)r], zz.first, D, vp,
                                                                last, &st[(size_t)r]);
                  t[(size_t)r] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                } catch (const std::exception& e) {
                  err[(size_t)r] = e.what();
                }
              });
            for (auto& x : th) x.join();
            for (auto& e : err)
              if (!e.empty()) throw std::runtime_error("run_volume_slabs_threads: " + e);
            if (rep > 0) walls.push_back(*std::max_element(t.begin(), t.end()));
          }
        }
        py::dict d;
        d["walls_s"] = walls;
        std::vector<int> rounds;
        std::vector<int64_t> bytes;
        std::vector<uint8_t> region, dilated;
        for (int r = 0; r < nranks; ++r) {
          rounds.push_back(st[(size_t)r].rounds);
          bytes.push_back(st[(size_t)r].exchanged_bytes);
          region.insert(region.end(), res[(size_t)r].region.begin(), res[(size_t)r].region.end());
          dilated.insert(dilated.end(), res[(size_t)r].dilated.begin(), res[(size_t)r].dilated.end());
        }
        d["rounds"] = rounds;
        d["exchanged_bytes"] = bytes;
        d["region"] = to_np<uint8_t>(region, {D, H, W});
        d["dilated"] = to_np<uint8_t>(dilated, {D, H, W});
        return d;
      },
      py::arg("volume"), py::arg("nranks"), py::arg("params") = PipelineParams(), py::arg("connectivity") = 6,
      py::arg("dilation") = 7, py::arg("device") = 0, py::arg("repeats") = 5);

  // The same decomposition on the golden model: this rank's slab of a band volume (0/1 uint8,
  // planes [z0, z0 + d) of `depth`), seeds in volume coordinates. Collective over `comm`.
  m.def(
      "golden_volume_slab",
      [](Comm& comm, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> band, int z0, int depth,
         const std::vector<std::tuple<int, int, int>>& seeds, int connectivity, int dilation) {
        if (band.ndim() != 3) throw std::invalid_argument("band must be (depth, height, width)");
        const int d = (int)band.shape(0), h = (int)band.shape(1), w = (int)band.shape(2);
        GoldenSlabGrower g(from_np<uint8_t>(band), w, h, d, slab_seeds(seeds_from(seeds), w, h, depth, z0, d),
                           connectivity);
        SlabStats st;
        {
          py::gil_scoped_release nogil;
          st = grow_and_dilate_slabs(comm, g, w, h, depth, z0, z0 + d, connectivity, dilation);
        }
        py::dict r;
        r["region"] = to_np<uint8_t>(g.region(), {d, h, w});
        r["dilated"] = to_np<uint8_t>(g.dilated(), {d, h, w});
        r["rounds"] = st.rounds;
        r["exchanged_bytes"] = st.exchanged_bytes;
        return r;
      },
      py::arg("comm"), py::arg("band"), py::arg("z0"), py::arg("depth"), py::arg("seeds"), py::arg("connectivity") = 6,
      py::arg("dilation") = 7);
  // CPU self-test of the decomposition: `ranks` forked rank processes over the host comm (no HIP),
  // each growing its slab of `band` on the golden model; returns the reassembled (region,
  // dilated, rounds) — to compare with the single-volume golden result.
  m.def(
      "golden_slabs_selftest",
      [](int ranks, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> band,
         const std::vector<std::tuple<int, int, int>>& seeds, int connectivity, int dilation) {
        if (band.ndim() != 3) throw std::invalid_argument("band must be (depth, height, width)");
        const int D = (int)band.shape(0), h = (int)band.shape(1), w = (int)band.shape(2);
        const size_t vox = (size_t)D * h * w;
        const std::vector<uint8_t> b = from_np<uint8_t>(band);
        const std::vector<Seed> sd = seeds_from(seeds);
        // Results come back through a shared anonymous mapping made before the fork.
        void* map = mmap(nullptr, 2 * vox + 64, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
        if (map == MAP_FAILED) throw std::runtime_error("mmap failed");
        auto* out = static_cast<uint8_t*>(map);
        LaunchOptions o;
        o.comm = "host";
        o.timeout_s = 60;
        int rc;
        {
          py::gil_scoped_release nogil;
          rc = launch_ranks(ranks, [&](int rank, int size, Comm& c) {
            const auto [z0, z1] = slab_bounds(D, rank, size);
            const size_t plane = (size_t)w * h;
            GoldenSlabGrower g(std::vector<uint8_t>(b.begin() + (long)(z0 * plane), b.begin() + (long)(z1 * plane)), w, h,
                               z1 - z0, slab_seeds(sd, w, h, D, z0, z1 - z0), connectivity);
            const SlabStats st = grow_and_dilate_slabs(c, g, w, h, D, z0, z1, connectivity, dilation);
            std::memcpy(out + z0 * plane, g.region().data(), g.region().size());
            std::memcpy(out + vox + z0 * plane, g.dilated().data(), g.dilated().size());
            if (rank == 0) std::memcpy(out + 2 * vox, &st.rounds, sizeof(int));
            return 0;
          }, o);
        }
        std::vector<uint8_t> reg(out, out + vox), dil(out + vox, out + 2 * vox);
        int rounds = 0;
        std::memcpy(&rounds, out + 2 * vox, sizeof(int));
        munmap(map, 2 * vox + 64);
        if (rc != 0) throw std::runtime_error("golden_slabs_selftest: a rank failed with status " + std::to_string(rc));
        return py::make_tuple(to_np<uint8_t>(reg, {D, h, w}), to_np<uint8_t>(dil, {D, h, w}), rounds);
      },
      py::arg("ranks"), py::arg("band"), py::arg("seeds"), py::arg("connectivity") = 6, py::arg("dilation") = 7);

  // ---- raw-pointer kernel entry points (torch interop; all synchronous on `stream`) ----------------
  m.def("k_threshold", [](uintptr_t in, uintptr_t out, size_t n, float lo, float hi, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    gpu::launch_threshold((const float*)in, (uint8_t*)out, n, lo, hi, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_threshold");
  });
  m.def("k_median", [](uintptr_t raw, uintptr_t out, int n, int h, int w, int k, const std::string& type, int stored_bits,
                       uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    BatchTables t = upload_tables(n, h, w, parse_type(type), stored_bits, 1.f, 0.f, {}, st);
    gpu::launch_median((const uint16_t*)raw, (uint16_t*)out, t.desc, t.medt, t.nmed, k, t.stats, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_median");
  });
  m.def("k_sharpen_band", [](uintptr_t med, uintptr_t band, uintptr_t sharp, int n, int h, int w, const std::string& type,
                             int stored_bits, float slope, float intercept, const PipelineParams& p, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    BatchTables t = upload_tables(n, h, w, parse_type(type), stored_bits, slope, intercept, {}, st);
    gpu::launch_sharpen_band((const uint16_t*)med, (uint64_t*)band, (float*)sharp, t.desc, t.shpt, t.nshp,
                             consts_from(p, 2), t.stats, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_sharpen_band");
  });
  m.def("k_srg_morph", [](uintptr_t band, uintptr_t region, uintptr_t dilated, uintptr_t eroded, uintptr_t border_region,
                          int n, int h, int w, const std::vector<std::tuple<int, int, int>>& seeds, const PipelineParams& p,
                          int border_radius, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    BatchTables t = upload_tables(n, h, w, kU16, 16, 1.f, 0.f, seeds_from(seeds), st);
    gpu::SrgOutputs o;
    o.region = (uint64_t*)region;
    o.dilated = (uint64_t*)dilated;
    o.eroded = (uint64_t*)eroded;
    o.border_region = (uint64_t*)border_region;
    void* scr = nullptr;  // bit planes of slices above the LDS limit
    if (w > gpu::kSrgMaxDim || h > gpu::kSrgMaxDim) {
      gpu::check_hip(hipMalloc(&scr, (size_t)n * 4 * gpu::srg_plane_words(w, h) * 8), "hipMalloc srg scratch");
      o.scratch = (uint64_t*)scr;
    }
    try {
      gpu::launch_srg_morph((const uint64_t*)band, t.desc, n, t.seeds, consts_from(p, border_radius), o, w, h, st);
      gpu::check_hip(hipStreamSynchronize(st), "k_srg_morph");
    } catch (...) {
      if (scr) {
        (void)hipStreamSynchronize(st);
        (void)hipFree(scr);
      }
      throw;
    }
    if (scr) (void)hipFree(scr);
  });
  // 3D region growing on bit volumes [d][h][ceil(w/64)] (int64 words), continuing from the region
  // already present when reset is false; returns the sweep count. Synchronous on `stream`.
  m.def("k_srg3d", [](uintptr_t band, uintptr_t region, int w, int h, int d,
                      const std::vector<std::tuple<int, int, int>>& seeds, int connectivity, bool reset,
                      uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("connectivity must be 6 or 26");
    std::vector<int32_t> sx;
    for (const auto& [x, y, z] : seeds) {
      sx.push_back(x);
      sx.push_back(y);
      sx.push_back(z);
    }
    int32_t* d_seeds = nullptr;
    uint32_t* d_flag = nullptr;
    uint32_t* h_flag = nullptr;
    uint64_t* scratch = nullptr;
    auto release = [&] {
      if (d_seeds) (void)hipFree(d_seeds);
      if (d_flag) (void)hipFree(d_flag);
      if (h_flag) (void)hipHostFree(h_flag);
      if (scratch) (void)hipFree(scratch);
    };
    try {
      gpu::check_hip(hipMalloc((void**)&d_flag, gpu::kSrg3dCtlWords * sizeof(uint32_t)), "hipMalloc flag");
      gpu::check_hip(hipHostMalloc((void**)&h_flag, gpu::kSrg3dCtlWords * sizeof(uint32_t), hipHostMallocDefault),
                     "hipHostMalloc flag");
      if (const size_t sw = gpu::srg3d_scratch_words(w, h, d))
        gpu::check_hip(hipMalloc((void**)&scratch, sw * 8), "hipMalloc srg3d scratch");
      if (!sx.empty()) {
        gpu::check_hip(hipMalloc((void**)&d_seeds, sx.size() * sizeof(int32_t)), "hipMalloc seeds");
        gpu::check_hip(hipMemcpyAsync(d_seeds, sx.data(), sx.size() * sizeof(int32_t), hipMemcpyHostToDevice, st),
                       "H2D seeds");
      }
      gpu::srg_volume((const uint64_t*)band, (uint64_t*)region, w, h, d, d_seeds, (int)(sx.size() / 3), connectivity,
                      d_flag, h_flag, scratch, st, reset);
      gpu::check_hip(hipStreamSynchronize(st), "k_srg3d");
      const int sweeps = gpu::srg_volume_result(h_flag);
      release();
      return sweeps;
    } catch (...) {
      (void)hipStreamSynchronize(st);
      release();
      throw;
    }
  });
  m.def("k_dilate3d", [](uintptr_t src, uintptr_t dst, uintptr_t tmp, int w, int h, int d, int size, uintptr_t stream,
                         bool ball) {
    hipStream_t st = as_stream(stream);
    if (size < 1 || size > gpu::kMorph3dMaxSize || !(size & 1))
      throw std::invalid_argument("dilation size must be odd and in [1, " + std::to_string(gpu::kMorph3dMaxSize) + "]");
    void* scr = nullptr;
    if (const size_t sw = gpu::morph3d_scratch_words(w, h, d))
      gpu::check_hip(hipMalloc(&scr, sw * 8), "hipMalloc morph scratch");
    try {
      gpu::dilate_volume((const uint64_t*)src, (uint64_t*)dst, (uint64_t*)tmp, w, h, d, size, st, (uint64_t*)scr, ball);
      gpu::check_hip(hipStreamSynchronize(st), "k_dilate3d");
    } catch (...) {
      (void)hipStreamSynchronize(st);
      if (scr) (void)hipFree(scr);
      throw;
    }
    if (scr) (void)hipFree(scr);
  }, py::arg("src"), py::arg("dst"), py::arg("tmp"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("size"),
     py::arg("stream"), py::arg("ball") = false);
  // Per-plane renderer border (label ∧ ¬erode of the (2·radius + 1)² square) of a bit volume.
  m.def("k_border3d", [](uintptr_t src, uintptr_t dst, int w, int h, int d, int radius, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (radius < 0 || 2 * radius + 1 > gpu::kMorph3dMaxSize)
      throw std::invalid_argument("border radius must be in [0, " + std::to_string(gpu::kMorph3dMaxSize / 2) + "]");
    void* scr = nullptr;
    if (const size_t sw = gpu::morph3d_scratch_words(w, h, d))
      gpu::check_hip(hipMalloc(&scr, sw * 8), "hipMalloc morph scratch");
    try {
      gpu::border_volume((const uint64_t*)src, (uint64_t*)dst, w, h, d, radius, st, (uint64_t*)scr);
      gpu::check_hip(hipStreamSynchronize(st), "k_border3d");
    } catch (...) {
      (void)hipStreamSynchronize(st);
      if (scr) (void)hipFree(scr);
      throw;
    }
    if (scr) (void)hipFree(scr);
  });
  m.def("k_jpeg", [](uintptr_t canvas, int n, int h, int w, int quality, uintptr_t stream, int sampling) {
    hipStream_t st = as_stream(stream);
    const int blocks = (w / 8) * (h / 8);
    const uint32_t out_cap = 512 * 1024 + 64;
    std::vector<gpu::JpegDesc> jd(n);
    for (int i = 0; i < n; ++i) {
      std::memset(&jd[i], 0, sizeof(jd[i]));
      jd[i].canvas_off = (uint32_t)((size_t)i * w * h);
      jd[i].out_off = (uint64_t)i * out_cap;
      jd[i].out_cap = out_cap;
      jd[i].render = -1;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
      size_t o = off;
      off += (bytes + 255) / 256 * 256;
      return o;
    };
    const size_t look_cap = (size_t)n * ((blocks + 255) / 256);
    const size_t o_jd = take(sizeof(gpu::JpegDesc) * n), o_look = take(6 * look_cap * 8), o_ticket = take(4 * (size_t)n),
                 o_spill = take(look_cap * 256 * 56 * 4), o_out = take((size_t)n * out_cap), o_sz = take((size_t)n * 4);
    uint8_t* dev = (uint8_t*)scratch().get(off);
    gpu::check_hip(hipMemcpyAsync(dev + o_jd, jd.data(), sizeof(gpu::JpegDesc) * n, hipMemcpyHostToDevice, st), "H2D");
    gpu::check_hip(hipMemsetAsync(dev + o_ticket, 0, 4 * (size_t)n, st), "memset tickets");
    gpu::check_hip(hipMemsetAsync(dev + o_look, 0, 6 * look_cap * 8, st), "memset look-back");
    gpu::JpegWork wk;
    wk.look = (uint64_t*)(dev + o_look);
    wk.look_cap = look_cap;
    wk.ticket = (uint32_t*)(dev + o_ticket);
    wk.spill = (uint32_t*)(dev + o_spill);
    int32_t divs[64];
    gpu::jpeg_divisors(quality, divs);
    gpu::launch_jpeg((const uint8_t*)canvas, (const gpu::JpegDesc*)(dev + o_jd), n, w, h, divs, wk, dev + o_out,
                     (int32_t*)(dev + o_sz), st, nullptr, sampling);
    std::vector<int32_t> sizes(n);
    gpu::check_hip(hipMemcpyAsync(sizes.data(), dev + o_sz, 4 * n, hipMemcpyDeviceToHost, st), "D2H");
    gpu::check_hip(hipStreamSynchronize(st), "k_jpeg");
    py::list res;
    for (int i = 0; i < n; ++i) {
      if (sizes[i] < 0) {
        res.append(py::none());
        continue;
      }
      std::string b((size_t)sizes[i], '\0');
      gpu::check_hip(hipMemcpy(b.data(), dev + o_out + (size_t)i * out_cap, sizes[i], hipMemcpyDeviceToHost), "D2H");
      res.append(py::bytes(b));
    }
    return res;
  }, py::arg("canvas"), py::arg("n"), py::arg("h"), py::arg("w"), py::arg("quality"), py::arg("stream"),
     py::arg("sampling") = 0);

  // Colour encoder on RGB canvases [n, h, w, 3] (device pointer); `out_cap` bytes per image (0: the
  // canvas size, which no baseline scan of 8-bit samples exceeds in practice). None for an image
  // that overflowed.
  m.def("k_jpeg_rgb", [](uintptr_t canvas, int n, int h, int w, int quality, uintptr_t stream, int sampling,
                         uint32_t out_cap) {
    hipStream_t st = as_stream(stream);
    if (sampling != 0 && sampling != 1) throw std::invalid_argument("a colour image needs sampling 0 (4:2:0) or 1 (4:4:4)");
    if (n <= 0 || h <= 0 || w <= 0 || h % 16 || w % 16) throw std::invalid_argument("canvas dims must be multiples of 16");
    if ((size_t)n * h * w * 3 > 0xFFFFFFFFull) throw std::invalid_argument("canvases exceed 4 GiB");
    {
      // The colour encoder's code object, loaded on the current device before this op's first launch
      // there (once per device: a process may use the op on several).
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_jpeg_rgb();
        preloaded.push_back(dev);
      }
    }
    if (!out_cap) out_cap = (uint32_t)((size_t)h * w * 3 + 1024);
    out_cap = (out_cap + 15u) & ~15u;
    std::vector<gpu::JpegDesc> jd(n);
    for (int i = 0; i < n; ++i) {
      std::memset(&jd[i], 0, sizeof(jd[i]));
      jd[i].canvas_off = (uint32_t)((size_t)i * w * h * 3);
      jd[i].out_off = (uint64_t)i * out_cap;
      jd[i].out_cap = out_cap;
      jd[i].render = -1;
    }
    size_t off = 0;
    auto take = [&](size_t bytes) {
      size_t o = off;
      off += (bytes + 255) / 256 * 256;
      return o;
    };
    const size_t look_cap = (size_t)n * gpu::jpeg_rgb_parts(w, h, sampling);
    const size_t o_jd = take(sizeof(gpu::JpegDesc) * n), o_look = take(6 * look_cap * 8), o_ticket = take(4 * (size_t)n),
                 o_spill = take(look_cap * 256 * 56 * 4), o_out = take((size_t)n * out_cap), o_sz = take((size_t)n * 4);
    uint8_t* dev = (uint8_t*)scratch().get(off);
    gpu::check_hip(hipMemcpyAsync(dev + o_jd, jd.data(), sizeof(gpu::JpegDesc) * n, hipMemcpyHostToDevice, st), "H2D");
    gpu::check_hip(hipMemsetAsync(dev + o_ticket, 0, 4 * (size_t)n, st), "memset tickets");
    gpu::check_hip(hipMemsetAsync(dev + o_look, 0, 6 * look_cap * 8, st), "memset look-back");
    gpu::JpegWork wk;
    wk.look = (uint64_t*)(dev + o_look);
    wk.look_cap = look_cap;
    wk.ticket = (uint32_t*)(dev + o_ticket);
    wk.spill = (uint32_t*)(dev + o_spill);
    const jpeg::Tables t = jpeg::make_tables(quality);
    gpu::launch_jpeg_rgb((const uint8_t*)canvas, (const gpu::JpegDesc*)(dev + o_jd), n, w, h, t.div_luma, t.div_chroma, wk,
                         dev + o_out, (int32_t*)(dev + o_sz), st, sampling);
    std::vector<int32_t> sizes(n);
    gpu::check_hip(hipMemcpyAsync(sizes.data(), dev + o_sz, 4 * n, hipMemcpyDeviceToHost, st), "D2H");
    gpu::check_hip(hipStreamSynchronize(st), "k_jpeg_rgb");
    py::list res;
    for (int i = 0; i < n; ++i) {
      if (sizes[i] < 0) {
        res.append(py::none());
        continue;
      }
      std::string b((size_t)sizes[i], '\0');
      gpu::check_hip(hipMemcpy(b.data(), dev + o_out + (size_t)i * out_cap, sizes[i], hipMemcpyDeviceToHost), "D2H");
      res.append(py::bytes(b));
    }
    return res;
  }, py::arg("canvas"), py::arg("n"), py::arg("h"), py::arg("w"), py::arg("quality"), py::arg("stream"),
     py::arg("sampling") = 0, py::arg("out_cap") = 0);
  // Overlay render of n equally sized slices: raw [n, h, w] u16, planes [2, n, h, wpr] u64 words
  // (label, then border), per-slice raw key range (the render window) → rgb [n, out_h, out_w, 3].
  m.def("k_render_overlay", [](uintptr_t raw, uintptr_t planes, uintptr_t rgb, int n, int h, int w, const std::string& type,
                               int stored_bits, float slope, float intercept, float sx, float sy, int out_w, int out_h,
                               bool nearest, int fill_a, int border_a, const std::vector<int>& color,
                               const std::vector<uint32_t>& key_min, const std::vector<uint32_t>& key_max, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (n <= 0 || (int)key_min.size() != n || (int)key_max.size() != n) throw std::invalid_argument("one key range per slice");
    if (color.size() != 3) throw std::invalid_argument("color must have three values");
    if (out_w <= 0 || out_h <= 0 || out_w % 4) throw std::invalid_argument("canvas width must be a multiple of 4");
    if (w <= 0 || h <= 0 || w > 0xFFFF || h > 0xFFFF) throw std::invalid_argument("bad slice size");
    const PixelType pt = parse_type(type);
    const int wpr = (w + 63) / 64;
    const RenderGeom g = make_render_geom(w, h, sx, sy, out_w, out_h);
    std::vector<gpu::RenderDesc> rd(2 * (size_t)n);
    std::vector<gpu::SliceStats> stats(n);
    for (int i = 0; i < n; ++i) {
      gpu::RenderDesc r;
      std::memset(&r, 0, sizeof(r));
      r.kind = gpu::kRenderRawGray;
      r.type = pt == kU8 ? kU16 : pt;
      r.stored_bits = (uint8_t)stored_bits;
      r.fill = (uint8_t)fill_a;
      r.border_value = (uint8_t)border_a;
      r.filter = nearest ? 1 : 0;
      r.slice = (uint32_t)i;
      r.src_w = (uint16_t)w;
      r.src_h = (uint16_t)h;
      r.wpr = (uint16_t)wpr;
      r.ox = g.ox;
      r.oy = g.oy;
      r.invx = g.invx;
      r.invy = g.invy;
      r.slope = slope;
      r.intercept = intercept;
      r.src_off = (uint32_t)((size_t)i * h * w);
      rd[i] = r;
      r.kind = gpu::kRenderLabels;
      r.src_off = (uint32_t)((size_t)i * h * wpr);
      r.border_off = (uint32_t)(((size_t)n + i) * h * wpr);
      rd[(size_t)n + i] = r;
      stats[i] = gpu::SliceStats{key_min[i], key_max[i], 0xFFFFFFFFu, 0u};
    }
    const size_t o_rd = 0, o_st = (rd.size() * sizeof(gpu::RenderDesc) + 255) / 256 * 256,
                 total = o_st + stats.size() * sizeof(gpu::SliceStats);
    std::vector<uint8_t> blob(total);
    std::memcpy(blob.data() + o_rd, rd.data(), rd.size() * sizeof(gpu::RenderDesc));
    std::memcpy(blob.data() + o_st, stats.data(), stats.size() * sizeof(gpu::SliceStats));
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::check_hip(hipMemcpyAsync(dev, blob.data(), total, hipMemcpyHostToDevice, st), "H2D tables");
    gpu::check_hip(hipStreamSynchronize(st), "sync tables");
    const uint32_t col = (uint32_t)(color[0] & 255) | ((uint32_t)(color[1] & 255) << 8) | ((uint32_t)(color[2] & 255) << 16);
    gpu::launch_render_overlay((const uint16_t*)raw, nullptr, (const uint64_t*)planes, (const gpu::SliceStats*)(dev + o_st),
                               (const gpu::RenderDesc*)(dev + o_rd), 0, n, 1, n, out_w, out_h, col, (uint8_t*)rgb, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_render_overlay");
  });

  // K7 on a batch of slices of ANY sizes in one launch: planes = the dilated planes of every slice
  // back to back (slice i: hs[i] × ceil(ws[i] / 64) words), then the region planes in the same layout;
  // raw = the slices' u16 samples back to back. Returns one record dict per slice.
  m.def("k_measure", [](uintptr_t planes, uintptr_t raw, const std::vector<int>& hs, const std::vector<int>& ws,
                        const std::string& type, int stored_bits, int connectivity, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    const int n = (int)hs.size();
    if (n <= 0 || ws.size() != hs.size()) throw std::invalid_argument("one height and one width per slice");
    if (connectivity != 4 && connectivity != 8) throw std::invalid_argument("connectivity must be 4 or 8");
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    const PixelType pt = parse_type(type);
    {
      // K7's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_measure();
        preloaded.push_back(dev);
      }
    }
    std::vector<gpu::SliceDesc> d((size_t)n);
    size_t raw_off = 0, mask_off = 0;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
      const int h = hs[(size_t)i], w = ws[(size_t)i];
      if (w <= 0 || h <= 0 || w > gpu::kMaxSliceDim || h > gpu::kMaxSliceDim) throw std::invalid_argument("bad slice size");
      gpu::SliceDesc& s = d[(size_t)i];
      std::memset(&s, 0, sizeof(s));
      s.raw_off = (uint32_t)raw_off;
      s.mask_off = (uint32_t)mask_off;
      s.w = (uint16_t)w;
      s.h = (uint16_t)h;
      s.wpr = (uint16_t)((w + 63) / 64);
      s.type = pt == kU8 ? kU16 : pt;
      s.stored_bits = (uint8_t)stored_bits;
      raw_off += (size_t)h * w;
      mask_off += (size_t)h * s.wpr;
      max_w = std::max(max_w, w);
      max_h = std::max(max_h, h);
    }
    if (raw_off > 0xFFFFFFFFull) throw std::invalid_argument("batch exceeds 2^32 samples");
    const size_t per = gpu::measure_scratch_words(max_w, max_h);
    const size_t o_desc = 0, o_out = (sizeof(gpu::SliceDesc) * n + 255) / 256 * 256,
                 o_par = (o_out + sizeof(SliceMeasure) * n + 255) / 256 * 256, total = o_par + per * n * sizeof(uint32_t);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::check_hip(hipMemcpyAsync(dev + o_desc, d.data(), sizeof(gpu::SliceDesc) * n, hipMemcpyHostToDevice, st), "H2D descriptors");
    gpu::check_hip(hipStreamSynchronize(st), "sync descriptors");
    const uint64_t* pl = (const uint64_t*)planes;
    gpu::launch_measure(pl, pl + mask_off, (const uint16_t*)raw, (const gpu::SliceDesc*)(dev + o_desc), n, connectivity,
                        (SliceMeasure*)(dev + o_out), (uint32_t*)(dev + o_par), max_w, max_h, st);
    std::vector<SliceMeasure> res((size_t)n);
    gpu::check_hip(hipMemcpyAsync(res.data(), dev + o_out, sizeof(SliceMeasure) * n, hipMemcpyDeviceToHost, st), "D2H records");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure");
    py::list out;
    for (auto& r : res) out.append(measure_dict(r));
    return out;
  }, py::arg("planes"), py::arg("raw"), py::arg("hs"), py::arg("ws"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
     py::arg("connectivity") = 8, py::arg("stream") = 0);

  // K7 then K9 on a batch of masks of ANY sizes, one launch each: planes = the masks' bit planes back to
  // back (mask i: hs[i] × ceil(ws[i] / 64) words); raw = at least Σ hs[i] · ws[i] u16 samples for K7's
  // intensity figures (their values do not matter here). Returns one diameter record dict per mask.
  m.def("k_measure_diameters", [](uintptr_t planes, uintptr_t raw, const std::vector<int>& hs, const std::vector<int>& ws,
                                  int connectivity, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    const int n = (int)hs.size();
    if (n <= 0 || ws.size() != hs.size()) throw std::invalid_argument("one height and one width per mask");
    if (connectivity != 4 && connectivity != 8) throw std::invalid_argument("connectivity must be 4 or 8");
    {
      // K7's and K9's code objects, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_measure();
        gpu::preload_measure_diameters();
        preloaded.push_back(dev);
      }
    }
    std::vector<gpu::SliceDesc> d((size_t)n);
    size_t raw_off = 0, mask_off = 0;
    int max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
      const int h = hs[(size_t)i], w = ws[(size_t)i];
      if (w <= 0 || h <= 0 || w > gpu::kMaxSliceDim || h > gpu::kMaxSliceDim) throw std::invalid_argument("bad mask size");
      gpu::SliceDesc& s = d[(size_t)i];
      std::memset(&s, 0, sizeof(s));
      s.raw_off = (uint32_t)raw_off;
      s.mask_off = (uint32_t)mask_off;
      s.w = (uint16_t)w;
      s.h = (uint16_t)h;
      s.wpr = (uint16_t)((w + 63) / 64);
      s.type = kU16;
      s.stored_bits = 16;
      raw_off += (size_t)h * w;
      mask_off += (size_t)h * s.wpr;
      max_w = std::max(max_w, w);
      max_h = std::max(max_h, h);
    }
    if (raw_off > 0xFFFFFFFFull) throw std::invalid_argument("batch exceeds 2^32 samples");
    const size_t per = gpu::measure_scratch_words(max_w, max_h);
    const size_t o_desc = 0, o_out = (sizeof(gpu::SliceDesc) * n + 255) / 256 * 256,
                 o_dia = (o_out + sizeof(SliceMeasure) * n + 255) / 256 * 256,
                 o_par = (o_dia + sizeof(SliceDiameters) * n + 255) / 256 * 256, total = o_par + per * n * sizeof(uint32_t);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::check_hip(hipMemcpyAsync(dev + o_desc, d.data(), sizeof(gpu::SliceDesc) * n, hipMemcpyHostToDevice, st), "H2D descriptors");
    gpu::check_hip(hipStreamSynchronize(st), "sync descriptors");
    const uint64_t* pl = (const uint64_t*)planes;
    gpu::launch_measure(pl, pl, (const uint16_t*)raw, (const gpu::SliceDesc*)(dev + o_desc), n, connectivity,
                        (SliceMeasure*)(dev + o_out), (uint32_t*)(dev + o_par), max_w, max_h, st);
    gpu::launch_measure_diameters(pl, (const gpu::SliceDesc*)(dev + o_desc), n, (SliceDiameters*)(dev + o_dia),
                                  (const uint32_t*)(dev + o_par), max_w, max_h, st);
    std::vector<SliceDiameters> res((size_t)n);
    gpu::check_hip(hipMemcpyAsync(res.data(), dev + o_dia, sizeof(SliceDiameters) * n, hipMemcpyDeviceToHost, st), "D2H records");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_diameters");
    py::list out;
    for (auto& r : res) {
      if (r.lesion_px == kDiametersNotMeasured) throw std::runtime_error("k_measure_diameters: a mask was not measured");
      out.append(diameters_dict(r));
    }
    return out;
  }, py::arg("planes"), py::arg("raw"), py::arg("hs"), py::arg("ws"), py::arg("connectivity") = 8, py::arg("stream") = 0);

  // K8 on bit volumes [d][h][ceil(w/64)] (int64 words): `dilated` and `region`, the 16-bit samples
  // `raw` [d][h][w]. Returns the record dict. Synchronous on `stream`; the scratch is kept across calls.
  m.def("k_measure_volume", [](uintptr_t dilated, uintptr_t region, uintptr_t raw, int w, int h, int d,
                               const std::string& type, int stored_bits, int connectivity, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("connectivity must be 6 or 26");
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    const size_t slots = gpu::volume_measure_scratch_words(w, h, d);
    if (slots == 0) throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    const PixelType pt = parse_type(type);
    {
      // K8's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_measure();
        preloaded.push_back(dev);
      }
    }
    const size_t o_acc = 0, o_out = 256, o_par = 512, total = o_par + slots * sizeof(uint32_t);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::launch_volume_measure((const uint64_t*)dilated, (const uint64_t*)region, (const uint16_t*)raw, (size_t)w * h, w, h,
                               d, (uint8_t)(pt == kU8 ? kU16 : pt), (uint8_t)stored_bits, connectivity,
                               (uint32_t*)(dev + o_par), (uint64_t*)(dev + o_acc), (VolumeMeasure*)(dev + o_out), st);
    VolumeMeasure res;
    gpu::check_hip(hipMemcpyAsync(&res, dev + o_out, sizeof(VolumeMeasure), hipMemcpyDeviceToHost, st), "D2H record");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_volume");
    return volume_measure_dict(res);
  }, py::arg("dilated"), py::arg("region"), py::arg("raw"), py::arg("w"), py::arg("h"), py::arg("d"),
     py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("connectivity") = 26, py::arg("stream") = 0);

  // K8 with the K10 launches between its two passes: the record dict and the list of the lesion dicts
  // (the `max_lesions` largest components, largest first). Same arguments as k_measure_volume.
  m.def("k_measure_volume_lesions", [](uintptr_t dilated, uintptr_t region, uintptr_t raw, int w, int h, int d,
                                       int max_lesions, const std::string& type, int stored_bits, int connectivity,
                                       uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("connectivity must be 6 or 26");
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    check_max_lesions(max_lesions);
    const size_t slots = gpu::volume_measure_scratch_words(w, h, d);
    if (slots == 0) throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    const PixelType pt = parse_type(type);
    {
      // K8's and K10's code objects, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_measure();
        gpu::preload_volume_lesions();
        preloaded.push_back(dev);
      }
    }
    const size_t n_out = sizeof(VolumeLesion) * (size_t)(kMaxVolumeLesions + 1);  // records, then the count
    const size_t work = (gpu::volume_lesions_work_bytes(w, h, d, max_lesions) + 255) / 256 * 256;
    const size_t o_acc = 0, o_out = 256, o_les = 512, o_work = o_les + n_out, o_par = o_work + work,
                 total = o_par + slots * sizeof(uint32_t);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::VolumeLesionWork lw;
    lw.max_lesions = max_lesions;
    lw.work = dev + o_work;
    lw.out = (VolumeLesion*)(dev + o_les);
    lw.out_count = (uint32_t*)(dev + o_les + sizeof(VolumeLesion) * kMaxVolumeLesions);
    gpu::launch_volume_measure((const uint64_t*)dilated, (const uint64_t*)region, (const uint16_t*)raw, (size_t)w * h, w, h,
                               d, (uint8_t)(pt == kU8 ? kU16 : pt), (uint8_t)stored_bits, connectivity,
                               (uint32_t*)(dev + o_par), (uint64_t*)(dev + o_acc), (VolumeMeasure*)(dev + o_out), st, &lw);
    VolumeMeasure res;
    std::vector<VolumeLesion> les((size_t)kMaxVolumeLesions + 1);
    gpu::check_hip(hipMemcpyAsync(&res, dev + o_out, sizeof(VolumeMeasure), hipMemcpyDeviceToHost, st), "D2H record");
    gpu::check_hip(hipMemcpyAsync(les.data(), dev + o_les, n_out, hipMemcpyDeviceToHost, st), "D2H lesions");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_volume_lesions");
    const uint32_t count = *reinterpret_cast<const uint32_t*>(&les[(size_t)kMaxVolumeLesions]);
    if (count > (uint32_t)max_lesions) throw std::runtime_error("k_measure_volume_lesions: count out of range");
    return py::make_tuple(volume_measure_dict(res), volume_lesion_list(les.data(), count));
  }, py::arg("dilated"), py::arg("region"), py::arg("raw"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("max_lesions"),
     py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("connectivity") = 26, py::arg("stream") = 0);

  // K8 with the K10 and K13 launches between its two passes: (lesion dicts, diameter dicts), both in K10's
  // order. `raw` holds the samples K8 and K10 read; their values do not enter the diameters.
  m.def("k_measure_volume_diameters", [](uintptr_t dilated, uintptr_t raw, int w, int h, int d, int max_lesions,
                                         const std::vector<int64_t>& spacing_um, int connectivity, bool brute_force,
                                         uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("connectivity must be 6 or 26");
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    check_max_lesions(max_lesions);
    const size_t slots = gpu::volume_measure_scratch_words(w, h, d);
    if (slots == 0) throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    gpu::VolumeDiametersWork dw;
    spacing_um_from(spacing_um, dw.spacing_um);
    const std::string ext = measure::volume_diameters_extent_error(w, h, d, dw.spacing_um);
    if (!ext.empty()) throw std::invalid_argument(ext);
    {
      // K8's, K10's and K13's code objects, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_measure();
        gpu::preload_volume_lesions();
        gpu::preload_volume_diameters();
        preloaded.push_back(dev);
      }
    }
    const size_t n_out = sizeof(VolumeLesion) * (size_t)(kMaxVolumeLesions + 1);  // records, then the count
    const size_t n_dia = sizeof(VolumeLesionDiameters) * (size_t)kMaxVolumeLesions;
    const size_t work = (gpu::volume_lesions_work_bytes(w, h, d, max_lesions) + 255) / 256 * 256;
    const size_t dwork = (gpu::volume_diameters_work_bytes(w, h, d, max_lesions) + 255) / 256 * 256;
    const size_t o_acc = 0, o_out = 256, o_les = 512, o_dia = o_les + n_out, o_work = o_dia + n_dia, o_dwork = o_work + work,
                 o_par = o_dwork + dwork, total = o_par + slots * sizeof(uint32_t);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    dw.work = dev + o_dwork;
    dw.out = (VolumeLesionDiameters*)(dev + o_dia);
    dw.brute_force = brute_force;
    gpu::VolumeLesionWork lw;
    lw.max_lesions = max_lesions;
    lw.work = dev + o_work;
    lw.out = (VolumeLesion*)(dev + o_les);
    lw.out_count = (uint32_t*)(dev + o_les + sizeof(VolumeLesion) * kMaxVolumeLesions);
    lw.diameters = &dw;
    gpu::launch_volume_measure((const uint64_t*)dilated, (const uint64_t*)dilated, (const uint16_t*)raw, (size_t)w * h, w, h, d,
                               (uint8_t)kU16, (uint8_t)16, connectivity, (uint32_t*)(dev + o_par), (uint64_t*)(dev + o_acc),
                               (VolumeMeasure*)(dev + o_out), st, &lw);
    std::vector<VolumeLesion> les((size_t)kMaxVolumeLesions + 1);
    std::vector<VolumeLesionDiameters> dia((size_t)kMaxVolumeLesions);
    gpu::check_hip(hipMemcpyAsync(les.data(), dev + o_les, n_out, hipMemcpyDeviceToHost, st), "D2H lesions");
    gpu::check_hip(hipMemcpyAsync(dia.data(), dev + o_dia, sizeof(VolumeLesionDiameters) * (size_t)max_lesions,
                                  hipMemcpyDeviceToHost, st), "D2H diameters");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_volume_diameters");
    const uint32_t count = *reinterpret_cast<const uint32_t*>(&les[(size_t)kMaxVolumeLesions]);
    if (count > (uint32_t)max_lesions) throw std::runtime_error("k_measure_volume_diameters: count out of range");
    return py::make_tuple(volume_lesion_list(les.data(), count), volume_diameters_list(dia.data(), count),
                          volume_diameters_list(dia.data() + count, (size_t)max_lesions - count));
  }, py::arg("dilated"), py::arg("raw"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("max_lesions"),
     py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000}, py::arg("connectivity") = 26,
     py::arg("brute_force") = false, py::arg("stream") = 0);

  // The golden views (nm03/volume_views.h) of the samples `raw` and the mask `dilated` ([D, H, W] each).
  m.def(
      "golden_volume_views",
      [](py::array_t<uint16_t, py::array::c_style | py::array::forcecast> raw,
         py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dilated, const py::object& at, const std::string& type,
         int stored_bits, bool inverted) {
        if (raw.ndim() != 3 || dilated.ndim() != 3) throw std::invalid_argument("raw and dilated must be [D, H, W]");
        for (int a = 0; a < 3; ++a)
          if (raw.shape(a) != dilated.shape(a)) throw std::invalid_argument("raw and dilated must have one shape");
        const PixelType pt = parse_type(type);
        const ViewsAt a = views_at_from(at);
        return views_dict(golden::volume_views(raw.data(), dilated.data(), (int)raw.shape(2), (int)raw.shape(1), (int)raw.shape(0),
                                               (uint8_t)pt, stored_bits, inverted, a));
      },
      py::arg("raw"), py::arg("dilated"), py::arg("at") = py::str("mask"), py::arg("type") = "u16", py::arg("stored_bits") = 16,
      py::arg("inverted") = false);
  // The sidecar text of a views dict (golden_volume_views, k_volume_views, VolumeRunner.export_views).
  m.def(
      "volume_views_to_json",
      [](const py::dict& v, double sx, double sy, double sz) { return views::to_json(views_from(v), (float)sx, (float)sy, sz); },
      py::arg("views"), py::arg("spacing_x") = 1.0, py::arg("spacing_y") = 1.0, py::arg("spacing_z") = 1.0);
  // The twelve files of a views dict that holds its planes, by the host renderer and encoder: file name → bytes.
  m.def(
      "golden_volume_view_jpegs",
      [](const py::dict& v, const RenderParams& rp, const std::vector<double>& spacing, const std::string& type, int stored_bits,
         float slope, float intercept) {
        if (spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
        if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
        const VolumeViews vv = views_from(v);
        for (int i = 0; i < kVolumeViewCount; ++i)
          if (vv.view[i].raw.size() != (size_t)vv.view[i].w * vv.view[i].h || vv.view[i].mask.size() != vv.view[i].raw.size())
            throw std::invalid_argument("views: every view needs its raw and mask planes");
        const PixelType pt = parse_type(type);
        std::vector<std::vector<uint8_t>> files;
        {
          py::gil_scoped_release nogil;
          files = golden::volume_view_jpegs(vv, (uint8_t)pt, stored_bits, slope, intercept, (float)spacing[0], (float)spacing[1],
                                            spacing[2], rp);
        }
        return view_files_dict(files);
      },
      py::arg("views"), py::arg("render") = RenderParams(), py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0},
      py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("slope") = 1.f, py::arg("intercept") = 0.f);

  // K14 alone on device tensors: `raw` the 16-bit samples (plane z at raw + z · plane_stride), `dilated` the
  // bit volume [d][h][ceil(w/64)] (int64 words). Returns the views dict with its planes. Synchronous on `stream`.
  m.def("k_volume_views", [](uintptr_t raw, uintptr_t dilated, int w, int h, int d, int64_t plane_stride, const py::object& at,
                             const std::string& type, int stored_bits, bool inverted, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    if (plane_stride < (int64_t)w * h) throw std::invalid_argument("plane_stride must be at least w * h");
    if ((uint64_t)plane_stride * (uint64_t)d > 0xFFFFFFFFull) throw std::invalid_argument("volume too large: plane_stride * d must stay below 2^32");
    const PixelType pt = parse_type(type);
    const ViewsAt a = views_at_from(at);
    const std::string err = views::at_error(a, w, h, d);
    if (!err.empty()) throw std::invalid_argument(err);
    {
      // K14's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_views();
        preloaded.push_back(dev);
      }
    }
    const gpu::VolumeViewsLayout L = gpu::volume_views_layout(w, h, d);
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t o_head = 0, o_samples = up(sizeof(gpu::VolumeViewsHead)), o_bits = o_samples + up(L.samples * 2),
                 o_proj = o_bits + up(L.bit_words * 8), total = o_proj + up(L.proj * 4);
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::launch_volume_views((const uint16_t*)raw, (size_t)plane_stride, (const uint64_t*)dilated, (uint8_t)pt, (uint8_t)stored_bits,
                             inverted, a, L, (uint16_t*)(dev + o_samples), (uint64_t*)(dev + o_bits), (uint32_t*)(dev + o_proj),
                             (gpu::VolumeViewsHead*)(dev + o_head), st);
    gpu::VolumeViewsHead hh;
    std::vector<uint16_t> hs(L.samples);
    std::vector<uint64_t> hb(L.border_off);
    gpu::check_hip(hipMemcpyAsync(&hh, dev + o_head, sizeof(hh), hipMemcpyDeviceToHost, st), "D2H views head");
    gpu::check_hip(hipMemcpyAsync(hs.data(), dev + o_samples, hs.size() * 2, hipMemcpyDeviceToHost, st), "D2H view samples");
    gpu::check_hip(hipMemcpyAsync(hb.data(), dev + o_bits, hb.size() * 8, hipMemcpyDeviceToHost, st), "D2H view masks");
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_views");
    VolumeViews r;
    r.w = w, r.h = h, r.d = d;
    r.at_mode = a.mode;
    r.inverted = inverted;
    r.has_box = hh.has_box != 0;
    for (int k = 0; k < 3; ++k) r.at[k] = hh.at[k];
    for (int k = 0; k < 6; ++k) r.box[k] = hh.box[k];
    const uint8_t t = pt == kU8 ? (uint8_t)kU16 : (uint8_t)pt;
    for (int i = 0; i < kVolumeViewCount; ++i) {
      VolumeView& q = r.view[i];
      q.w = L.vw[i];
      q.h = L.vh[i];
      q.raw_min = (int32_t)raw_value_from_key((uint16_t)hh.stats[i].key_min, t);
      q.raw_max = (int32_t)raw_value_from_key((uint16_t)hh.stats[i].key_max, t);
      q.mask_px = hh.mask_px[i];
      q.raw.assign(hs.begin() + L.sample_off[i], hs.begin() + L.sample_off[i] + (size_t)q.w * q.h);
      q.mask.assign((size_t)q.w * q.h, 0);
      for (int y = 0; y < q.h; ++y)
        for (int x = 0; x < q.w; ++x) q.mask[(size_t)y * q.w + x] = (hb[L.mask_off[i] + (size_t)y * L.wpr[i] + x / 64] >> (x % 64)) & 1;
    }
    return views_dict(r);
  }, py::arg("raw"), py::arg("dilated"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("plane_stride"),
     py::arg("at") = py::str("mask"), py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("inverted") = false,
     py::arg("stream") = 0);

  // The golden surface mesh (nm03/volume_mesh.h) of the mask `dilated` ([D, H, W], non-zero = set).
  m.def(
      "golden_volume_mesh",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dilated, const std::vector<double>& spacing,
         const std::string& placement) {
        if (dilated.ndim() != 3) throw std::invalid_argument("dilated must be [D, H, W]");
        if (spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
        const int pl = mesh_placement_from(placement);
        VolumeMesh r;
        {
          py::gil_scoped_release nogil;
          r = golden::volume_mesh(dilated.data(), (int)dilated.shape(2), (int)dilated.shape(1), (int)dilated.shape(0),
                                  (float)spacing[0], (float)spacing[1], spacing[2], pl);
        }
        return mesh_dict(r);
      },
      py::arg("dilated"), py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0}, py::arg("placement") = "corner");
  // The same mesh from the K15 kernels' per-word functions and blocked scan, run on the host
  // (measure::volume_mesh_words): what the kernels compute, without a GPU.
  m.def(
      "volume_mesh_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> dilated, const std::vector<double>& spacing,
         const std::string& placement, int scan_block) {
        if (dilated.ndim() != 3) throw std::invalid_argument("dilated must be [D, H, W]");
        if (spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
        const int pl = mesh_placement_from(placement);
        const std::vector<uint64_t> dw = pack_volume(dilated);
        VolumeMesh r;
        {
          py::gil_scoped_release nogil;
          r = measure::volume_mesh_words(dw.data(), (int)dilated.shape(2), (int)dilated.shape(1), (int)dilated.shape(0),
                                         (float)spacing[0], (float)spacing[1], spacing[2], pl, scan_block);
        }
        return mesh_dict(r);
      },
      py::arg("dilated"), py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0}, py::arg("placement") = "corner",
      py::arg("scan_block") = 0);
  // (default, smallest, largest) scan block of K15 in lattice words, and the lattice words of a volume.
  m.def("volume_mesh_scan_blocks", [] { return py::make_tuple(mesh::kScanBlock, mesh::kMinScanBlock, mesh::kMaxScanBlock); });
  // Empty, or why a mesh of V vertices and Q quads is refused under a cap of max_bytes.
  m.def("volume_mesh_size_error", [](uint64_t V, uint64_t Q, uint64_t max_bytes) { return mesh::size_error(V, Q, max_bytes); });
  // The bytes of mesh.ply / mesh.stl of a mesh dict, by the one writer.
  m.def(
      "volume_mesh_file",
      [](const py::dict& md, const std::string& format) {
        const VolumeMesh vm = mesh_from(md);
        const std::vector<uint8_t> b = mesh::file_bytes(vm, mesh_format_from(format));
        return py::bytes((const char*)b.data(), b.size());
      },
      py::arg("mesh"), py::arg("format") = "ply");
  // The text of mesh.json for a mesh dict whose file has `bytes` bytes.
  m.def(
      "volume_mesh_to_json",
      [](const py::dict& md, const std::string& format, uint64_t bytes, const std::vector<double>& spacing) {
        if (spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
        return mesh::to_json(mesh_from(md), mesh_format_from(format), bytes, (float)spacing[0], (float)spacing[1], spacing[2]);
      },
      py::arg("mesh"), py::arg("format") = "ply", py::arg("bytes") = 0, py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0});

  // K15 alone on a device bit volume [d][h][ceil(w/64)] (int64 words). Returns the mesh dict. One host round
  // trip between the scan and the emission; synchronous on `stream`.
  m.def("k_volume_mesh", [](uintptr_t dilated, int w, int h, int d, const std::vector<double>& spacing, const std::string& placement,
                            int scan_block, uint64_t max_bytes, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (spacing.size() != 3) throw std::invalid_argument("spacing must be (sx, sy, sz)");
    const int pl = mesh_placement_from(placement);
    if (scan_block != 0 && (scan_block < mesh::kMinScanBlock || scan_block > mesh::kMaxScanBlock))
      throw std::invalid_argument("scan_block must be 0 (default) or " + std::to_string(mesh::kMinScanBlock) + " .. " +
                                  std::to_string(mesh::kMaxScanBlock));
    {
      // K15's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_mesh();
        preloaded.push_back(dev);
      }
    }
    const gpu::VolumeMeshLayout L = gpu::volume_mesh_layout(w, h, d, scan_block);
    struct DevMem {  // this op's own buffers: the shared scratch may be regrown between the two halves
      void* p = nullptr;
      ~DevMem() {
        if (p) (void)hipFree(p);
      }
    } work, out;
    gpu::check_hip(hipMalloc(&work.p, L.bytes), "hipMalloc mesh work");
    gpu::VolumeMeshHead* h_head = nullptr;
    gpu::check_hip(hipHostMalloc((void**)&h_head, sizeof(gpu::VolumeMeshHead), hipHostMallocDefault), "hipHostMalloc mesh head");
    struct Pinned {
      void* p;
      ~Pinned() { (void)hipHostFree(p); }
    } pinned{h_head};
    gpu::launch_volume_mesh((const uint64_t*)dilated, L, work.p, h_head, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_mesh totals");
    const gpu::VolumeMeshHead hh = *h_head;
    const uint64_t nv = hh.total[0], nq = hh.total[1] + hh.total[2] + hh.total[3];
    const std::string err = mesh::size_error(nv, nq, max_bytes);
    if (!err.empty()) throw std::runtime_error(err);
    VolumeMesh r;
    r.w = w, r.h = h, r.d = d;
    r.placement = pl;
    r.quads_x = hh.total[1], r.quads_y = hh.total[2], r.quads_z = hh.total[3];
    r.voxels = hh.voxels;
    r.positions.resize(3 * (size_t)nv);
    r.quads.resize(4 * (size_t)nq);
    const size_t pos_bytes = (12 * (size_t)nv + 255) / 256 * 256;
    gpu::check_hip(hipMalloc(&out.p, std::max<size_t>(pos_bytes + 16 * (size_t)nq, 256)), "hipMalloc mesh result");
    float* d_pos = (float*)out.p;
    uint32_t* d_quads = (uint32_t*)((uint8_t*)out.p + pos_bytes);
    gpu::launch_volume_mesh_emit((const uint64_t*)dilated, L, work.p, hh, pl, (float)spacing[0], (float)spacing[1], (float)spacing[2],
                                 d_pos, d_quads, st);
    if (nv) gpu::check_hip(hipMemcpyAsync(r.positions.data(), d_pos, 12 * (size_t)nv, hipMemcpyDeviceToHost, st), "D2H mesh positions");
    if (nq) gpu::check_hip(hipMemcpyAsync(r.quads.data(), d_quads, 16 * (size_t)nq, hipMemcpyDeviceToHost, st), "D2H mesh quads");
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_mesh");
    return mesh_dict(r);
  }, py::arg("dilated"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing") = std::vector<double>{1.0, 1.0, 1.0},
     py::arg("placement") = "corner", py::arg("scan_block") = 0, py::arg("max_bytes") = mesh::kDefaultMaxMb << 20,
     py::arg("stream") = 0);

  // ---- K16: the distance map of nm03/volume_distance.h -------------------------------------------------
  // The golden map (whole-line minima) of `mask` ([D, H, W], non-zero = set) → int64 [D, H, W].
  m.def(
      "golden_volume_distance",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, const std::vector<int64_t>& spacing_um,
         bool to_background, const py::object& cap_um) {
        uint32_t um[3];
        distance_args(mask, spacing_um, um);
        const int64_t cap = cap_um.is_none() ? -1 : cap_um.cast<int64_t>();
        if (!cap_um.is_none() && cap < 0) throw std::invalid_argument("cap_um must not be negative");
        const int d = (int)mask.shape(0), h = (int)mask.shape(1), w = (int)mask.shape(2);
        const std::vector<uint8_t> mk = from_np<uint8_t>(mask);
        std::vector<int64_t> r;
        {
          py::gil_scoped_release nogil;
          r = golden::volume_distance(mk, w, h, d, um, to_background, cap);
        }
        return to_np<int64_t>(r, {d, h, w});
      },
      py::arg("mask"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000}, py::arg("to_background") = false,
      py::arg("cap_um") = py::none());
  // The golden margin by the direct definition → uint8 [D, H, W].
  m.def(
      "golden_dilate3d_mm",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> region, const std::vector<int64_t>& spacing_um,
         int64_t radius_um) {
        uint32_t um[3];
        distance_args(region, spacing_um, um);
        const int d = (int)region.shape(0), h = (int)region.shape(1), w = (int)region.shape(2);
        const std::vector<uint8_t> mk = from_np<uint8_t>(region);
        std::vector<uint8_t> r;
        {
          py::gil_scoped_release nogil;
          r = golden::dilate3d_mm(mk, w, h, d, um, radius_um);
        }
        return to_np<uint8_t>(r, {d, h, w});
      },
      py::arg("region"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000}, py::arg("radius_um") = 0);
  // The golden thickness → the thickness dict (inscribed_um2, inscribed_at, found, inscribed_radius_mm, thickness_mm).
  m.def(
      "golden_volume_thickness",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, const std::vector<int64_t>& spacing_um) {
        uint32_t um[3];
        distance_args(mask, spacing_um, um);
        const int d = (int)mask.shape(0), h = (int)mask.shape(1), w = (int)mask.shape(2);
        const std::vector<uint8_t> mk = from_np<uint8_t>(mask);
        VolumeThickness t;
        {
          py::gil_scoped_release nogil;
          t = golden::volume_thickness(mk, w, h, d, um);
        }
        return volume_thickness_dict(t);
      },
      py::arg("mask"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000});
  // The map and the thickness from the K16 kernels' per-line functions run on the host
  // (measure::volume_distance_words): what the kernels compute, without a GPU. `junk`: the storage bits past
  // the width are set, as a kernel may find them.
  m.def(
      "volume_distance_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, const std::vector<int64_t>& spacing_um,
         bool to_background, const py::object& cap_um, bool junk) {
        uint32_t um[3];
        distance_args(mask, spacing_um, um);
        const int64_t cap = cap_um.is_none() ? -1 : cap_um.cast<int64_t>();
        if (!cap_um.is_none() && cap < 0) throw std::invalid_argument("cap_um must not be negative");
        const int d = (int)mask.shape(0), h = (int)mask.shape(1), w = (int)mask.shape(2), wpr = (w + 63) / 64;
        std::vector<uint64_t> words = pack_volume(mask);
        if (junk)
          for (size_t r = 0; r < (size_t)d * h; ++r) words[r * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, w);
        std::vector<int64_t> out((size_t)w * h * d);
        {
          py::gil_scoped_release nogil;
          measure::volume_distance_words(words.data(), w, h, d, wpr, um, to_background, cap, out.data());
        }
        return to_np<int64_t>(out, {d, h, w});
      },
      py::arg("mask"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000}, py::arg("to_background") = false,
      py::arg("cap_um") = py::none(), py::arg("junk") = false);
  m.def(
      "volume_thickness_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask, const std::vector<int64_t>& spacing_um) {
        uint32_t um[3];
        distance_args(mask, spacing_um, um);
        const int d = (int)mask.shape(0), h = (int)mask.shape(1), w = (int)mask.shape(2), wpr = (w + 63) / 64;
        const std::vector<uint64_t> words = pack_volume(mask);
        VolumeThickness t;
        {
          py::gil_scoped_release nogil;
          t = measure::volume_thickness_words(words.data(), w, h, d, wpr, um);
        }
        return volume_thickness_dict(t);
      },
      py::arg("mask"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000});
  // Empty, or why a w × h × d volume at (ux, uy, uz) is refused by the extent rule.
  m.def("volume_distance_extent_error", [](int w, int h, int d, const std::vector<int64_t>& spacing_um) {
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    return measure::volume_distance_extent_error(w, h, d, um);
  });
  // `text` (a volume sidecar) with the thickness keys of a thickness dict at (ux, uy, uz).
  m.def("volume_insert_thickness_keys", [](const std::string& text, const py::dict& thickness, const std::vector<int64_t>& spacing_um) {
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    return measure::insert_thickness_keys(text, volume_thickness_from(thickness), um);
  });
  // llround(R · 1000): the margin of --dilate-mm in micrometres.
  m.def("dilate_mm_to_um", [](double mm) { return measure::dilate_mm_to_um(mm); });
  m.attr("NO_DISTANCE") = py::int_(kNoDistance);

  // K16 alone on a device bit volume [d][h][ceil(w/64)] (int64 words). mode "map": `out` is int64 [d][h][w];
  // "margin": `out` is a bit volume like `bits`, `cap_um` the radius; "thickness": returns the dict. The work
  // buffer is this op's own; synchronous on `stream`.
  m.def("k_volume_distance", [](uintptr_t bits, int w, int h, int d, const std::vector<int64_t>& spacing_um, const std::string& mode,
                                bool to_background, int64_t cap_um, uintptr_t out, uintptr_t stream) -> py::object {
    hipStream_t st = as_stream(stream);
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    const std::string ext = measure::volume_distance_extent_error(w, h, d, um);
    if (!ext.empty()) throw std::invalid_argument(ext);
    if (mode != "map" && mode != "margin" && mode != "thickness") throw std::invalid_argument("mode must be map, margin or thickness");
    if (mode == "margin" && cap_um < 0) throw std::invalid_argument("the radius must not be negative");
    {
      // K16's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_distance();
        preloaded.push_back(dev);
      }
    }
    const gpu::VolumeDistanceLayout L = gpu::volume_distance_layout(w, h, d);
    struct DevMem {
      void* p = nullptr;
      ~DevMem() {
        if (p) (void)hipFree(p);
      }
    } work;
    gpu::check_hip(hipMalloc(&work.p, L.bytes), "hipMalloc distance work");
    if (mode == "map") {
      gpu::launch_volume_distance((const uint64_t*)bits, L, um, to_background, cap_um, work.p, (int64_t*)out, st);
      gpu::check_hip(hipStreamSynchronize(st), "k_volume_distance");
      return py::none();
    }
    if (mode == "margin") {
      gpu::launch_volume_margin((const uint64_t*)bits, L, um, cap_um, work.p, (uint64_t*)out, st);
      gpu::check_hip(hipStreamSynchronize(st), "k_volume_distance margin");
      return py::none();
    }
    VolumeThickness* h_rec = nullptr;
    gpu::check_hip(hipHostMalloc((void**)&h_rec, sizeof(VolumeThickness), hipHostMallocDefault), "hipHostMalloc thickness");
    struct Pinned {
      void* p;
      ~Pinned() { (void)hipHostFree(p); }
    } pinned{h_rec};
    gpu::launch_volume_thickness((const uint64_t*)bits, L, um, work.p, h_rec, st);
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_distance thickness");
    return volume_thickness_dict(*h_rec);
  }, py::arg("bits"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing_um"), py::arg("mode") = "map",
     py::arg("to_background") = false, py::arg("cap_um") = -1, py::arg("out") = 0, py::arg("stream") = 0);

  // ---- K17: the comparison of nm03/volume_compare.h ------------------------------------------------------
  // The golden comparison (plain loops, a sort) of two masks ([D, H, W], non-zero = set) → the dict of integers.
  m.def(
      "golden_compare_volumes",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b,
         const std::vector<int64_t>& spacing_um) {
        uint32_t um[3];
        compare_args(a, b, spacing_um, um);
        const int d = (int)a.shape(0), h = (int)a.shape(1), w = (int)a.shape(2);
        const std::vector<uint8_t> ma = from_np<uint8_t>(a), mb = from_np<uint8_t>(b);
        VolumeCompare c;
        {
          py::gil_scoped_release nogil;
          c = golden::compare_volumes(ma, mb, w, h, d, um);
        }
        return volume_compare_dict(c);
      },
      py::arg("a"), py::arg("b"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000});
  // S(M) of the golden model → uint8 [D, H, W].
  m.def("golden_volume_surface", [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> mask) {
    if (mask.ndim() != 3) throw std::invalid_argument("mask must be [D, H, W]");
    const int d = (int)mask.shape(0), h = (int)mask.shape(1), w = (int)mask.shape(2);
    return to_np<uint8_t>(golden::volume_surface(from_np<uint8_t>(mask), w, h, d), {d, h, w});
  });
  // The comparison from the K17 kernels' functions run on the host (measure::volume_compare_words). `junk`: the
  // storage bits past the width are set in both inputs. With `surfaces` the result is (dict, S(A), S(B)), the
  // surfaces as the int64 words [D, H, ceil(W / 64)] the surface launch stores.
  m.def(
      "volume_compare_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b,
         const std::vector<int64_t>& spacing_um, bool junk, bool surfaces) -> py::object {
        uint32_t um[3];
        compare_args(a, b, spacing_um, um);
        const int d = (int)a.shape(0), h = (int)a.shape(1), w = (int)a.shape(2), wpr = (w + 63) / 64;
        std::vector<uint64_t> wa = pack_volume(a), wb = pack_volume(b);
        if (junk)
          for (size_t r = 0; r < (size_t)d * h; ++r) {
            wa[r * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, w);
            wb[r * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, w);
          }
        std::vector<uint64_t> sa(wa.size()), sb(wb.size());
        VolumeCompare c;
        {
          py::gil_scoped_release nogil;
          c = measure::volume_compare_words(wa.data(), wb.data(), w, h, d, wpr, um, sa.data(), sb.data());
        }
        if (!surfaces) return volume_compare_dict(c);
        std::vector<int64_t> ia(sa.begin(), sa.end()), ib(sb.begin(), sb.end());
        return py::make_tuple(volume_compare_dict(c), to_np<int64_t>(ia, {d, h, wpr}), to_np<int64_t>(ib, {d, h, wpr}));
      },
      py::arg("a"), py::arg("b"), py::arg("spacing_um") = std::vector<int64_t>{1000, 1000, 1000}, py::arg("junk") = false,
      py::arg("surfaces") = false);
  // compare.json of a comparison dict: the one writer (compare::to_json).
  // `lesions`: None, or a lesion-wise comparison dict (golden_compare_volume_lesions), whose keys follow assd_mm.
  m.def("volume_compare_to_json", [](const py::dict& c, int w, int h, int d, const std::vector<int64_t>& spacing_um, const std::string& reference,
                                     const py::object& lesions) {
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    const OptionalLesions ol(lesions);
    return compare::to_json(volume_compare_from(c), w, h, d, um, reference, ol.get());
  }, py::arg("compare"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing_um"), py::arg("reference") = "",
     py::arg("lesions") = py::none());
  m.def("volume_compare_csv_header", [](bool lesions) { return compare::csv_header(lesions); }, py::arg("lesions") = false);
  m.def("volume_compare_csv_fields", [](const py::dict& c, int w, int h, int d, const std::vector<int64_t>& spacing_um, const std::string& reference,
                                        const py::object& lesions) {
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    const OptionalLesions ol(lesions);
    return compare::csv_fields(volume_compare_from(c), w, h, d, um, reference, ol.get());
  }, py::arg("compare"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing_um"), py::arg("reference") = "",
     py::arg("lesions") = py::none());
  // compare_lesions.csv: the header line and one patient's rows (compare::lesions_table_rows).
  m.def("volume_compare_lesions_table_header", []() { return compare::lesions_table_header(); });
  m.def("volume_compare_lesions_table_rows", [](const std::string& patient, const py::dict& lesions) {
    return compare::lesions_table_rows(patient, volume_compare_lesions_from(lesions));
  }, py::arg("patient"), py::arg("lesions"));
  // ⌊√v⌋ of the shared core (vcmp::isqrt_um), 0 ≤ v < 2^62.
  m.def("volume_compare_isqrt", [](int64_t v) {
    if (v < 0 || v >= (1ll << 62)) throw std::invalid_argument("0 <= v < 2^62");
    return vcmp::isqrt_um(v);
  });

  // ---- K18: the lesion-wise comparison of nm03/volume_compare_lesions.h ---------------------------------------
  // The golden model (flood fills, plain loops, a sort) on two masks ([D, H, W], non-zero = set) → the dict.
  m.def(
      "golden_compare_volume_lesions",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b,
         int max_lesions, int connectivity) {
        if (a.ndim() != 3) throw std::invalid_argument("mask must be [D, H, W]");
        if (b.ndim() != 3 || b.shape(0) != a.shape(0) || b.shape(1) != a.shape(1) || b.shape(2) != a.shape(2))
          throw std::invalid_argument("both masks must be [D, H, W] of one shape");
        const int d = (int)a.shape(0), h = (int)a.shape(1), w = (int)a.shape(2);
        const std::vector<uint8_t> ma = from_np<uint8_t>(a), mb = from_np<uint8_t>(b);
        VolumeCompareLesions l;
        {
          py::gil_scoped_release nogil;
          l = golden::compare_volume_lesions(ma, mb, w, h, d, max_lesions, connectivity);
        }
        return volume_compare_lesions_dict(l);
      },
      py::arg("a"), py::arg("b"), py::arg("max_lesions"), py::arg("connectivity") = 26);
  // The same from the K18 kernels' functions run on the host (measure::volume_compare_lesions_words). `junk`: the
  // storage bits past the width are set in both inputs.
  m.def(
      "volume_compare_lesions_words",
      [](py::array_t<uint8_t, py::array::c_style | py::array::forcecast> a, py::array_t<uint8_t, py::array::c_style | py::array::forcecast> b,
         int max_lesions, int connectivity, bool junk) {
        if (a.ndim() != 3) throw std::invalid_argument("mask must be [D, H, W]");
        if (b.ndim() != 3 || b.shape(0) != a.shape(0) || b.shape(1) != a.shape(1) || b.shape(2) != a.shape(2))
          throw std::invalid_argument("both masks must be [D, H, W] of one shape");
        const int d = (int)a.shape(0), h = (int)a.shape(1), w = (int)a.shape(2), wpr = (w + 63) / 64;
        std::vector<uint64_t> wa = pack_volume(a), wb = pack_volume(b);
        if (junk)
          for (size_t r = 0; r < (size_t)d * h; ++r) {
            wa[r * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, w);
            wb[r * wpr + wpr - 1] |= ~row_word_mask(wpr - 1, w);
          }
        VolumeCompareLesions l;
        {
          py::gil_scoped_release nogil;
          l = measure::volume_compare_lesions_words(wa.data(), wb.data(), w, h, d, wpr, max_lesions, connectivity);
        }
        return volume_compare_lesions_dict(l);
      },
      py::arg("a"), py::arg("b"), py::arg("max_lesions"), py::arg("connectivity") = 26, py::arg("junk") = false);

  // K18 alone on two device bit volumes [d][h][ceil(w/64)] (int64 words, bits past the width tolerated) → the dict.
  // The work buffer is this op's own; synchronous on `stream`. `max_blocks`: see launch_volume_compare_lesions.
  m.def("k_volume_compare_lesions", [](uintptr_t a, uintptr_t b, int w, int h, int d, int max_lesions, int connectivity, int max_blocks,
                                       uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (!a || !b) throw std::invalid_argument("null buffer");
    check_max_lesions(max_lesions);
    if (connectivity != 6 && connectivity != 26) throw std::invalid_argument("connectivity must be 6 or 26");
    if (max_blocks < 0) throw std::invalid_argument("max_blocks must not be negative");
    if (gpu::volume_measure_scratch_words(w, h, d) == 0)
      throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    {
      // K18's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_compare_lesions();
        preloaded.push_back(dev);
      }
    }
    struct DevMem {
      void* p = nullptr;
      ~DevMem() {
        if (p) (void)hipFree(p);
      }
    } work;
    gpu::check_hip(hipMalloc(&work.p, gpu::volume_compare_lesions_work_bytes(w, h, d, max_lesions)), "hipMalloc lesion comparison work");
    void* h_rec = nullptr;
    gpu::check_hip(hipHostMalloc(&h_rec, volume_compare_lesions_record_bytes(max_lesions), hipHostMallocDefault),
                   "hipHostMalloc lesion comparison");
    struct Pinned {
      void* p;
      ~Pinned() { (void)hipHostFree(p); }
    } pinned{h_rec};
    gpu::launch_volume_compare_lesions((const uint64_t*)a, (const uint64_t*)b, w, h, d, max_lesions, connectivity, work.p, h_rec, st, max_blocks);
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_compare_lesions");
    return volume_compare_lesions_dict(measure::unpack_compare_lesions(h_rec, max_lesions));
  }, py::arg("a"), py::arg("b"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("max_lesions"), py::arg("connectivity") = 26,
     py::arg("max_blocks") = 0, py::arg("stream") = 0);

  // K17 alone on two device bit volumes [d][h][ceil(w/64)] (int64 words) → the dict of integers. The work buffer
  // is this op's own; synchronous on `stream`. `max_blocks`: see launch_volume_compare.
  m.def("k_volume_compare", [](uintptr_t a, uintptr_t b, int w, int h, int d, const std::vector<int64_t>& spacing_um, int max_blocks,
                               uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (!a || !b) throw std::invalid_argument("null buffer");
    if (max_blocks < 0) throw std::invalid_argument("max_blocks must not be negative");
    uint32_t um[3];
    spacing_um_from(spacing_um, um);
    const std::string ext = measure::volume_distance_extent_error(w, h, d, um);
    if (!ext.empty()) throw std::invalid_argument(ext);
    {
      // K16's and K17's code objects, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_distance();
        gpu::preload_volume_compare();
        preloaded.push_back(dev);
      }
    }
    const gpu::VolumeCompareLayout L = gpu::volume_compare_layout(w, h, d);
    struct DevMem {
      void* p = nullptr;
      ~DevMem() {
        if (p) (void)hipFree(p);
      }
    } work;
    gpu::check_hip(hipMalloc(&work.p, L.bytes), "hipMalloc compare work");
    VolumeCompare* h_rec = nullptr;
    gpu::check_hip(hipHostMalloc((void**)&h_rec, sizeof(VolumeCompare), hipHostMallocDefault), "hipHostMalloc compare");
    struct Pinned {
      void* p;
      ~Pinned() { (void)hipHostFree(p); }
    } pinned{h_rec};
    gpu::launch_volume_compare((const uint64_t*)a, (const uint64_t*)b, L, um, work.p, h_rec, st, max_blocks);
    gpu::check_hip(hipStreamSynchronize(st), "k_volume_compare");
    return volume_compare_dict(*h_rec);
  }, py::arg("a"), py::arg("b"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("spacing_um"), py::arg("max_blocks") = 0,
     py::arg("stream") = 0);

  // K11 on a batch of masks of ANY sizes in one launch: planes = the masks' bit planes back to back
  // (mask i: hs[i] × ceil(ws[i] / 64) words); raw = the slices' u16 samples back to back; one pixel type
  // and stored_bits per mask (the descriptors carry them). Returns one intensity record dict per mask.
  m.def("k_measure_intensity", [](uintptr_t planes, uintptr_t raw, const std::vector<int>& hs, const std::vector<int>& ws,
                                  const std::vector<std::string>& types, const std::vector<int>& stored_bits,
                                  uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    const int n = (int)hs.size();
    if (n <= 0 || ws.size() != hs.size()) throw std::invalid_argument("one height and one width per mask");
    if (types.size() != hs.size() || stored_bits.size() != hs.size())
      throw std::invalid_argument("one pixel type and one stored_bits per mask");
    for (int b : stored_bits)
      if (b < 1 || b > 16) throw std::invalid_argument("stored_bits must be 1..16");
    {
      // K11's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_measure_intensity();
        preloaded.push_back(dev);
      }
    }
    std::vector<gpu::SliceDesc> d((size_t)n);
    size_t raw_off = 0, mask_off = 0;
    for (int i = 0; i < n; ++i) {
      const int h = hs[(size_t)i], w = ws[(size_t)i];
      if (w <= 0 || h <= 0 || w > gpu::kMaxSliceDim || h > gpu::kMaxSliceDim) throw std::invalid_argument("bad mask size");
      gpu::SliceDesc& s = d[(size_t)i];
      std::memset(&s, 0, sizeof(s));
      s.raw_off = (uint32_t)raw_off;
      s.mask_off = (uint32_t)mask_off;
      s.w = (uint16_t)w;
      s.h = (uint16_t)h;
      s.wpr = (uint16_t)((w + 63) / 64);
      const PixelType pt = parse_type(types[(size_t)i]);
      s.type = pt == kU8 ? kU16 : pt;
      s.stored_bits = (uint8_t)stored_bits[(size_t)i];
      raw_off += (size_t)h * w;
      mask_off += (size_t)h * s.wpr;
    }
    if (raw_off > 0xFFFFFFFFull) throw std::invalid_argument("batch exceeds 2^32 samples");
    const size_t o_desc = 0, o_out = (sizeof(gpu::SliceDesc) * n + 255) / 256 * 256, total = o_out + sizeof(IntensityStats) * n;
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::check_hip(hipMemcpyAsync(dev + o_desc, d.data(), sizeof(gpu::SliceDesc) * n, hipMemcpyHostToDevice, st), "H2D descriptors");
    gpu::check_hip(hipStreamSynchronize(st), "sync descriptors");
    gpu::launch_measure_intensity((const uint64_t*)planes, (const uint16_t*)raw, (const gpu::SliceDesc*)(dev + o_desc), n,
                                  (IntensityStats*)(dev + o_out), st);
    std::vector<IntensityStats> res((size_t)n);
    gpu::check_hip(hipMemcpyAsync(res.data(), dev + o_out, sizeof(IntensityStats) * n, hipMemcpyDeviceToHost, st), "D2H records");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_intensity");
    py::list out;
    for (auto& r : res) out.append(intensity_dict(r));
    return out;
  }, py::arg("planes"), py::arg("raw"), py::arg("hs"), py::arg("ws"), py::arg("types"), py::arg("stored_bits"),
     py::arg("stream") = 0);

  // K11's five 3D launches on a bit volume [d][h][ceil(w/64)] (int64 words) and the 16-bit samples `raw`
  // [d][h][w]. Returns the record dict. Synchronous on `stream`.
  m.def("k_measure_volume_intensity", [](uintptr_t dilated, uintptr_t raw, int w, int h, int d, const std::string& type,
                                         int stored_bits, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (gpu::volume_measure_scratch_words(w, h, d) == 0)
      throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    const PixelType pt = parse_type(type);
    {
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_intensity();
        preloaded.push_back(dev);
      }
    }
    const size_t o_out = 0, o_acc = 256, total = o_acc + gpu::kVolumeIntensityAccBytes;
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::launch_volume_intensity((const uint64_t*)dilated, (const uint16_t*)raw, (size_t)w * h, w, h, d,
                                 (uint8_t)(pt == kU8 ? kU16 : pt), (uint8_t)stored_bits, dev + o_acc,
                                 (IntensityStats*)(dev + o_out), st);
    IntensityStats res;
    gpu::check_hip(hipMemcpyAsync(&res, dev + o_out, sizeof(IntensityStats), hipMemcpyDeviceToHost, st), "D2H record");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_volume_intensity");
    return intensity_dict(res);
  }, py::arg("dilated"), py::arg("raw"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("type") = "u16",
     py::arg("stored_bits") = 16, py::arg("stream") = 0);

  // K12 on a batch of masks of ANY sizes in one launch (laid out as for k_measure_intensity), mask i at
  // levels[i] grey levels. Returns one texture record dict per mask.
  m.def("k_measure_texture", [](uintptr_t planes, uintptr_t raw, const std::vector<int>& hs, const std::vector<int>& ws,
                                const std::vector<int>& levels, const std::vector<std::string>& types,
                                const std::vector<int>& stored_bits, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    const int n = (int)hs.size();
    if (n <= 0 || ws.size() != hs.size()) throw std::invalid_argument("one height and one width per mask");
    if (types.size() != hs.size() || stored_bits.size() != hs.size() || levels.size() != hs.size())
      throw std::invalid_argument("one level count, one pixel type and one stored_bits per mask");
    for (int b : stored_bits)
      if (b < 1 || b > 16) throw std::invalid_argument("stored_bits must be 1..16");
    for (int l : levels)
      if (l < tcore::kMinLevels || l > tcore::kMaxLevels) throw std::invalid_argument("levels must be 2..64");
    {
      // K12's code object, loaded on the current device before this op's first launch there.
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_measure_texture();
        preloaded.push_back(dev);
      }
    }
    std::vector<gpu::SliceDesc> d((size_t)n);
    std::vector<gpu::TextureSlot> slots((size_t)n);
    size_t raw_off = 0, mask_off = 0, word_off = 0;
    for (int i = 0; i < n; ++i) {
      const int h = hs[(size_t)i], w = ws[(size_t)i];
      if (w <= 0 || h <= 0 || w > gpu::kMaxSliceDim || h > gpu::kMaxSliceDim) throw std::invalid_argument("bad mask size");
      gpu::SliceDesc& s = d[(size_t)i];
      std::memset(&s, 0, sizeof(s));
      s.raw_off = (uint32_t)raw_off;
      s.mask_off = (uint32_t)mask_off;
      s.w = (uint16_t)w;
      s.h = (uint16_t)h;
      s.wpr = (uint16_t)((w + 63) / 64);
      const PixelType pt = parse_type(types[(size_t)i]);
      s.type = pt == kU8 ? kU16 : pt;
      s.stored_bits = (uint8_t)stored_bits[(size_t)i];
      raw_off += (size_t)h * w;
      mask_off += (size_t)h * s.wpr;
      slots[(size_t)i].levels = (uint32_t)levels[(size_t)i];
      slots[(size_t)i].word_off = (uint32_t)word_off;  // records back to back: odd level counts leave them 4-byte aligned
      word_off += glcm_record_bytes(levels[(size_t)i]) / 4;
    }
    if (raw_off > 0xFFFFFFFFull) throw std::invalid_argument("batch exceeds 2^32 samples");
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t o_desc = 0, o_slots = up(sizeof(gpu::SliceDesc) * n), o_out = o_slots + up(sizeof(gpu::TextureSlot) * n),
                 out_bytes = word_off * 4, total = o_out + out_bytes;
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::check_hip(hipMemcpyAsync(dev + o_desc, d.data(), sizeof(gpu::SliceDesc) * n, hipMemcpyHostToDevice, st), "H2D descriptors");
    gpu::check_hip(hipMemcpyAsync(dev + o_slots, slots.data(), sizeof(gpu::TextureSlot) * n, hipMemcpyHostToDevice, st), "H2D slots");
    gpu::check_hip(hipStreamSynchronize(st), "sync descriptors");
    gpu::launch_measure_texture((const uint64_t*)planes, (const uint16_t*)raw, (const gpu::SliceDesc*)(dev + o_desc), n,
                                (const gpu::TextureSlot*)(dev + o_slots), 0, dev + o_out, st);
    std::vector<uint32_t> res(word_off);
    gpu::check_hip(hipMemcpyAsync(res.data(), dev + o_out, out_bytes, hipMemcpyDeviceToHost, st), "D2H records");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_texture");
    py::list out;
    for (int i = 0; i < n; ++i) out.append(texture_dict(measure::glcm_from_record(res.data() + slots[(size_t)i].word_off)));
    return out;
  }, py::arg("planes"), py::arg("raw"), py::arg("hs"), py::arg("ws"), py::arg("levels"), py::arg("types"),
     py::arg("stored_bits"), py::arg("stream") = 0);

  // K12's four 3D launches on a bit volume [d][h][ceil(w/64)] (int64 words) and the 16-bit samples `raw`
  // [d][h][w]. Returns the record dict. Synchronous on `stream`.
  m.def("k_measure_volume_texture", [](uintptr_t dilated, uintptr_t raw, int w, int h, int d, int levels,
                                       const std::string& type, int stored_bits, uintptr_t stream) {
    hipStream_t st = as_stream(stream);
    if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("stored_bits must be 1..16");
    if (levels < tcore::kMinLevels || levels > tcore::kMaxLevels) throw std::invalid_argument("levels must be 2..64");
    if (w <= 0 || h <= 0 || d <= 0) throw std::invalid_argument("empty volume");
    if (gpu::volume_measure_scratch_words(w, h, d) == 0)
      throw std::invalid_argument("volume too large to measure: (w + 1) * h * d + 1 must stay below 2^32");
    const PixelType pt = parse_type(type);
    {
      static std::mutex preload_m;
      static std::vector<int> preloaded;
      int dev = 0;
      gpu::check_hip(hipGetDevice(&dev), "hipGetDevice");
      std::lock_guard<std::mutex> g(preload_m);
      if (std::find(preloaded.begin(), preloaded.end(), dev) == preloaded.end()) {
        gpu::preload_volume_texture();
        preloaded.push_back(dev);
      }
    }
    const size_t rec = glcm_record_bytes(levels), o_out = 0, o_acc = (rec + 255) / 256 * 256,
                 total = o_acc + gpu::kVolumeTextureAccBytes;
    uint8_t* dev = (uint8_t*)scratch().get(total);
    gpu::launch_volume_texture((const uint64_t*)dilated, (const uint16_t*)raw, (size_t)w * h, w, h, d,
                               (uint8_t)(pt == kU8 ? kU16 : pt), (uint8_t)stored_bits, levels, dev + o_acc, dev + o_out, st);
    std::vector<uint32_t> res(rec / 4);
    gpu::check_hip(hipMemcpyAsync(res.data(), dev + o_out, rec, hipMemcpyDeviceToHost, st), "D2H record");
    gpu::check_hip(hipStreamSynchronize(st), "k_measure_volume_texture");
    const measure::Glcm g = measure::glcm_from_record(res.data());
    measure::check_glcm_exact(g.head.samples);
    return texture_dict(g);
  }, py::arg("dilated"), py::arg("raw"), py::arg("w"), py::arg("h"), py::arg("d"), py::arg("levels") = 32,
     py::arg("type") = "u16", py::arg("stored_bits") = 16, py::arg("stream") = 0);

  // ---- comm self-tests (CPU) ------------------------------------------------------------------------
  m.def("loopback_selftest", [](int n) {
    // Every rank contributes rank-dependent data; returns what rank 0 observed.
    auto group = make_loopback_group(n);
    std::vector<std::string> errors(n);
    std::vector<std::thread> th;
    for (int r = 0; r < n; ++r)
      th.emplace_back([&, r] {
        Comm& c = *group[r];
        try {
          std::vector<uint8_t> b;
          if (r == 0) b = {1, 2, 3, 4, 5};
          c.broadcast_bytes(b, 0);
          if (b != std::vector<uint8_t>{1, 2, 3, 4, 5}) errors[r] = "broadcast";
          std::vector<uint8_t> mine(r + 1, (uint8_t)r);
          auto all = c.allgather_bytes(mine);
          for (int q = 0; q < n; ++q)
            if (all[q] != std::vector<uint8_t>(q + 1, (uint8_t)q)) errors[r] = "allgather";
          int64_t v[2] = {r, 1};
          c.allreduce_sum_i64(v, 2);
          if (v[0] != (int64_t)n * (n - 1) / 2 || v[1] != n) errors[r] = "allreduce_sum";
          double f = r * 1.5;
          c.allreduce_max_f64(&f, 1);
          if (f != (n - 1) * 1.5) errors[r] = "allreduce_max";
          // ring neighbour exchange: send r+1 bytes up, receive r bytes from below (none at the ends)
          std::vector<uint8_t> up((size_t)r + 1, (uint8_t)(10 + r)), got((size_t)std::max(r, 0));
          c.sendrecv(up.data(), up.size(), r + 1 < n ? r + 1 : -1, got.data(), got.size(), r > 0 ? r - 1 : -1);
          if (r > 0 && got != std::vector<uint8_t>((size_t)r, (uint8_t)(9 + r))) errors[r] = "sendrecv";
          c.barrier();
        } catch (const std::exception& e) {
          errors[r] = e.what();
        }
      });
    for (auto& t : th) t.join();
    return errors;
  });
  m.def(
      "launcher_selftest",
      // Forks n rank processes over the host comm (no RCCL, no HIP): every rank checks the
      // collectives, then `mode` decides the ending — "ok": all succeed; "exit": the last rank
      // (n > 2) returns 7 after the collectives; "die": the last rank exits 3 while the others
      // block in a barrier (abort flag); "hang": the last rank sleeps while the others wait in
      // a barrier (deadline, then SIGTERM from the supervisor). Returns the job's exit status.
      // comm "rccl": the ranks get launch_ranks' deferred RCCL communicator; after the collectives each
      // starts RCCL and promotes — without a GPU every rank fails to bring RCCL up, they agree on it
      // and the last collectives run on the control plane.
      [](int n, const std::string& mode, double timeout_s, double grace_s, const std::string& comm) {
        LaunchOptions o;
        o.comm = comm;
        o.timeout_s = timeout_s;
        o.grace_s = grace_s;
        py::gil_scoped_release nogil;
        return launch_ranks(
            n,
            [mode](int rank, int size, Comm& c) {
              std::vector<uint8_t> b;
              if (rank == 0) b.assign(3 << 20, 0);  // larger than a slot: chunked broadcast
              for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(i * 7 + 1);
              c.broadcast_bytes(b, 0);
              for (size_t i = 0; i < b.size(); i += 4099)
                if (b[i] != (uint8_t)(i * 7 + 1)) return 11;
              if (b.size() != (3u << 20)) return 12;
              auto all = c.allgather_bytes(std::vector<uint8_t>(rank + 1, (uint8_t)rank));
              for (int q = 0; q < size; ++q)
                if (all[q] != std::vector<uint8_t>(q + 1, (uint8_t)q)) return 13;
              int64_t v[2] = {rank, 1};
              c.allreduce_sum_i64(v, 2);
              if (v[0] != (int64_t)size * (size - 1) / 2 || v[1] != size) return 14;
              double f = rank * 1.5;
              c.allreduce_max_f64(&f, 1);
              if (f != (size - 1) * 1.5) return 15;
              // neighbour exchange larger than a slot (chunked): rank r sends to r + 1
              const size_t big = (2u << 20) + 777;
              std::vector<uint8_t> snd(big), rcv(rank > 0 ? big : 0);
              for (size_t i = 0; i < big; ++i) snd[i] = (uint8_t)(i * 13 + rank);
              c.sendrecv(snd.data(), big, rank + 1 < size ? rank + 1 : -1, rcv.data(), rcv.size(), rank > 0 ? rank - 1 : -1);
              for (size_t i = 0; i < rcv.size(); i += 4097)
                if (rcv[i] != (uint8_t)(i * 13 + rank - 1)) return 16;
              const bool last = rank == size - 1;
              if (mode == "exit" && last && size > 2) return 7;
              if (mode == "die" && last) _exit(3);
              if (mode == "hang" && last) {
                std::this_thread::sleep_for(std::chrono::seconds(600));
                return 0;
              }
              c.start_data_plane();
              c.promote();  // ranks on different planes afterwards would hang the next collective
              int64_t one = 1;
              c.allreduce_sum_i64(&one, 1);
              if (one != size) return 18;
              c.barrier();
              return 0;
            },
            o);
      },
      py::arg("n"), py::arg("mode") = "exit", py::arg("timeout_s") = -1.0, py::arg("grace_s") = 5.0,
      py::arg("comm") = "host");

  // ---- native communicators (bench.py and other Python drivers) ------------------------------------
  // Host/RCCL comms for ranks started by torchrun or bench.py's own launcher; the rendezvous
  // (segment name or RCCL unique id) travels through the caller's store.
  py::class_<ShmSegment, std::shared_ptr<ShmSegment>>(m, "ShmSegment")
      .def_property_readonly("size", &ShmSegment::size)
      .def("wait_attached_and_unlink", [](ShmSegment& s, double t) {
        py::gil_scoped_release nogil;
        s.wait_attached_and_unlink(t);
      }, py::arg("timeout_s") = 120.0)
      .def("raise_abort", &ShmSegment::raise_abort)
      .def_property_readonly("aborted", &ShmSegment::aborted);
  m.def("shm_create", [](int n, std::string name) {
    auto s = ShmSegment::create_named(n, &name);
    return py::make_tuple(s, name);
  }, py::arg("n"), py::arg("name") = std::string());
  m.def("shm_attach", [](const std::string& name, int n, double t) {
    py::gil_scoped_release nogil;
    return ShmSegment::attach_named(name, n, t);
  }, py::arg("name"), py::arg("n"), py::arg("timeout_s") = 120.0);
  py::class_<Comm, std::unique_ptr<Comm>>(m, "Comm")
      .def_property_readonly("rank", &Comm::rank)
      .def_property_readonly("size", &Comm::size)
      .def_property_readonly("backend", [](const Comm& c) { return std::string(c.backend()); })
      .def("barrier", [](Comm& c) {
        py::gil_scoped_release nogil;
        c.barrier();
      })
      .def("broadcast_bytes", [](Comm& c, py::bytes data, int root) {
        std::string s = data;
        std::vector<uint8_t> v(s.begin(), s.end());
        {
          py::gil_scoped_release nogil;
          c.broadcast_bytes(v, root);
        }
        return py::bytes((const char*)v.data(), v.size());
      }, py::arg("data"), py::arg("root") = 0)
      .def("allgather_bytes", [](Comm& c, py::bytes data) {
        std::string s = data;
        std::vector<std::vector<uint8_t>> all;
        {
          py::gil_scoped_release nogil;
          all = c.allgather_bytes(std::vector<uint8_t>(s.begin(), s.end()));
        }
        py::list out;
        for (auto& v : all) out.append(py::bytes((const char*)v.data(), v.size()));
        return out;
      })
      .def("allreduce_sum", [](Comm& c, std::vector<int64_t> v) {
        py::gil_scoped_release nogil;
        c.allreduce_sum_i64(v.data(), v.size());
        return v;
      })
      .def("allreduce_max", [](Comm& c, std::vector<double> v) {
        py::gil_scoped_release nogil;
        c.allreduce_max_f64(v.data(), v.size());
        return v;
      })
      .def("start_data_plane", [](Comm& c) {
        py::gil_scoped_release nogil;
        c.start_data_plane();
      })
      .def("settle_data_plane", [](Comm& c) {
        py::gil_scoped_release nogil;
        c.settle_data_plane(nullptr);
      })
      .def("fail_data_plane", [](Comm& c, const std::string& why) { c.fail_data_plane(why); }, py::arg("why"))
      .def("promote", [](Comm& c) {
        py::gil_scoped_release nogil;
        c.promote();
      })
      .def_property_readonly("data_plane_times", [](const Comm& c) {
        const Comm::DataPlaneTimes t = c.data_plane_times();
        py::dict d;
        d["start_s"] = t.start_s;
        d["settle_s"] = t.settle_s;
        d["wait_s"] = t.wait_s;
        d["init_upper_s"] = t.init_upper_s;
        return d;
      })
      .def_property_readonly("fallback_error", &Comm::fallback_error)
      .def_property_readonly("transport_size", &Comm::transport_size)
      .def_property_readonly("transport_rank", &Comm::transport_rank)
      .def_property_readonly("transport_device", &Comm::transport_device)
      .def("set_abort_segment", &Comm::set_abort_segment, py::arg("segment"))
      .def("sendrecv", [](Comm& c, py::bytes data, int dst, size_t rbytes, int src) {
        std::string s = data;
        std::string out(rbytes, '\0');
        {
          py::gil_scoped_release nogil;
          c.sendrecv(s.data(), s.size(), dst, out.data(), rbytes, src);
        }
        return py::bytes(out);
      }, py::arg("data"), py::arg("dst"), py::arg("rbytes"), py::arg("src"))
      .def("gather_rank_devices", [](Comm& c, int device, const std::string& bus_id, int node, const std::string& cpus,
                                     int threads, const std::string& error) {
        RankDevice me;
        me.device = device;
        me.bus_id = bus_id;
        me.node = node;
        me.cpus = cpus;
        me.threads = threads;
        me.transport_size = c.transport_size();
        me.transport_device = c.transport_device();
        me.error = error;
        std::vector<RankDevice> all;
        {
          py::gil_scoped_release nogil;
          all = gather_rank_devices(c, me);
        }
        py::list out;
        for (const auto& d : all) {
          py::dict x;
          x["device"] = d.device;
          x["bus_id"] = d.bus_id;
          x["numa_node"] = d.node;
          x["cpus"] = d.cpus;
          x["threads"] = d.threads;
          x["transport_size"] = d.transport_size;
          x["transport_device"] = d.transport_device;
          x["error"] = d.error;
          out.append(x);
        }
        return out;
      }, py::arg("device"), py::arg("bus_id"), py::arg("node"), py::arg("cpus"), py::arg("threads"),
         py::arg("error") = "")
      .def("allgather_f64", [](Comm& c, std::vector<double> v) {
        std::vector<double> all(v.size() * (size_t)c.size());
        {
          py::gil_scoped_release nogil;
          c.allgather(v.data(), v.size() * sizeof(double), all.data());
        }
        return all;
      });
  m.def("self_comm", &make_self_comm);
  m.def("host_comm", [](std::shared_ptr<ShmSegment> seg, int rank, double t) { return make_host_comm(seg, rank, t); },
        py::arg("segment"), py::arg("rank"), py::arg("timeout_s") = -1.0);
  m.def("rccl_unique_id", [] {
    auto v = rccl_unique_id();
    return py::bytes((const char*)v.data(), v.size());
  });
  m.def("rccl_comm", [](int rank, int size, py::bytes uid, int device, std::shared_ptr<ShmSegment> seg, double t) {
    std::string s = uid;
    std::vector<uint8_t> v(s.begin(), s.end());
    py::gil_scoped_release nogil;
    return make_rccl_comm(rank, size, v, device, seg, t);
  }, py::arg("rank"), py::arg("size"), py::arg("unique_id"), py::arg("device"), py::arg("segment") = nullptr,
     py::arg("timeout_s") = -1.0);
  m.def("deferred_rccl_comm", [](int rank, int size, int device, std::shared_ptr<ShmSegment> seg, double t) {
    return make_deferred_rccl_comm(rank, size, device, std::move(seg), t);
  }, py::arg("rank"), py::arg("size"), py::arg("device"), py::arg("segment"), py::arg("timeout_s") = -1.0);
  m.def("comm_timeout_s", &comm_timeout_s);
  py::register_exception<CommError>(m, "CommError", PyExc_RuntimeError);
}
