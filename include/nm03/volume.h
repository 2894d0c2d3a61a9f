// nm03/volume.h — 3D mode (BASELINE config 5): a patient series loaded as one volume
// (the reference forces 2D with setLoadSeries(false), test_pipeline.cpp:38-41; FAST itself
// supports 3D SeededRegionGrowing/Dilation, which this mode provides on the GPU).
#pragma once

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "nm03/app.h"
#include "nm03/comm.h"
#include "nm03/engine.h"
#include "nm03/measure.h"
#include "nm03/volume_compare.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_distance.h"
#include "nm03/volume_mesh.h"
#include "nm03/volume_views.h"

namespace nm03 {

struct VolumeInput {
  int w = 0, h = 0, d = 0;
  PixelType type = kU16;
  int stored_bits = 16;
  float slope = 1.f, intercept = 0.f, spacing_x = 1.f, spacing_y = 1.f;
  // Distance between consecutive planes (mm) and where it came from (series_spacing_z).
  double spacing_z = 1.0;
  std::string spacing_z_source = "default";
  std::vector<uint16_t> raw;  // d planes of h×w
};

// The plane spacing of a series from the headers of its first two planes' files (`second`: nullptr
// when the first two planes come from one file, or there is one plane), by this rule, in order:
//   "position"                both files have ImagePositionPatient and the Euclidean distance between
//                             the two positions is > 0: that distance
//   "spacing_between_slices"  SpacingBetweenSlices (0018,0088) > 0
//   "slice_thickness"         SliceThickness (0018,0050) > 0
//   "default"                 1.0
// Whether the spacing is uniform over the series is not checked.
namespace dicom {
struct Header;
}
double series_spacing_z(const dicom::Header& first, const dicom::Header* second, std::string* source);

// Geometry of a series without its pixels (the first two files' headers): PixelSpacing and the plane
// spacing with its source, as load_volume sets them.
struct SeriesGeometry {
  float spacing_x = 1.f, spacing_y = 1.f;
  double spacing_z = 1.0;
  std::string spacing_z_source = "default";
};
SeriesGeometry series_geometry(const std::vector<std::string>& files);

// Load a series directory's slices (ordered like the 2D path) as a volume; all slices must share
// dimensions and pixel format.
VolumeInput load_volume(const std::vector<std::string>& files);

struct VolumeResult {
  int w = 0, h = 0, d = 0;
  int sweeps = 0;
  std::vector<uint8_t> band, region, dilated;  // 0/1 per voxel (when requested)
  double kernels_s = 0;
  VolumeMeasure measure = {};  // VolumeParams::measure: the K8 record of the dilated volume
  double measure_s = 0;        // GPU time of the K8 launches (outside kernels_s; the K10 launches included)
  // VolumeParams::measure_lesions: the K10 records of the largest components, largest first
  // (min(measure_lesions, measure.components) of them).
  std::vector<VolumeLesion> lesions;
  // VolumeParams::measure_diameters: the K13 records of the same lesions, in the same order.
  std::vector<VolumeLesionDiameters> diameters;
  // VolumeParams::measure_intensity: the K11 record of the samples under the dilated volume.
  IntensityStats intensity = {};
  // VolumeParams::measure_texture: the K12 record of the samples under the dilated volume.
  measure::Glcm texture;
  // VolumeParams::measure_thickness: the K16 record of the dilated volume.
  VolumeThickness thickness = {};
  // VolumeParams::compare: the K17 record of the dilated volume (A) against the reference (B), and the GPU time
  // of the reference upload and K17's launches (outside kernels_s and measure_s).
  VolumeCompare compare = {};
  double compare_s = 0;
  // VolumeParams::compare_lesions: the K18 record of the same two masks, and the GPU time of K18's launches
  // (outside compare_s).
  VolumeCompareLesions compare_lesions;
  double compare_lesions_s = 0;
};

// The reference mask of a comparison (VolumeParams::compare), in host memory, valid during run(): either `bits`
// (d planes of h rows of ceil(w / 64) u64 words, K5's layout, bits past the width tolerated) or `mask` (w · h · d
// bytes, non-zero = set, which the runner packs); `bits` wins when both are given.
struct VolumeReference {
  const uint64_t* bits = nullptr;
  const uint8_t* mask = nullptr;
  int w = 0, h = 0, d = 0;
};

struct VolumeExportStats {
  double export_s = 0;         // wall time of render + encode (GPU) incl. D2H of the JPEG bytes
  int64_t jpeg_fallbacks = 0;  // images re-encoded on the host (GPU capacity overflow)
};

// VolumeRunner::export_views: the views of nm03/volume_views.h, rendered and encoded.
struct VolumeViewsExport {
  // P, the box and every view's size, raw_min / raw_max and mask_px; the sample and mask planes only
  // when they were asked for (else empty).
  VolumeViews views;
  std::vector<std::vector<uint8_t>> files;  // the twelve JPEG files in views::file_name order
  double k14_s = 0;     // GPU time of K14's launches
  double render_s = 0;  // GPU time of the borders, K3 and K4 behind them
};

struct VolumeParams {
  PipelineParams pipe;        // median/sharpen/band per slice, then 3D SRG
  int connectivity = 6;       // 6 | 26
  int dilation_size = 7;      // cube edge (7×7×7 in config 5)
  bool preprocess = true;     // median + sharpen per slice before the band test
  std::vector<Seed> seeds;    // empty → reference seed pattern on the middle slice
  bool measure = false;           // also measure the dilated volume (K8, nm03/measure.h VolumeMeasure)
  int measure_connectivity = 26;  // 6 | 26: components; cavities use the dual
  // With measure: also one record per lesion for the N largest components (K10, nm03/measure.h
  // VolumeLesion); 0 = off, else 1 … kMaxVolumeLesions.
  int measure_lesions = 0;
  // With measure and measure_lesions ≥ 1: also the lengths of every reported lesion (K13, nm03/measure.h
  // VolumeLesionDiameters), maximised in `spacing_um` (x, y, z in integer micrometres,
  // measure::volume_spacing_um of the volume's spacing). A (dim − 1) · spacing_um ≥ 2^31 is refused.
  bool measure_diameters = false;
  uint32_t spacing_um[3] = {1000u, 1000u, 1000u};
  bool diameters_brute_force = false;  // K13 compares every tile pair: the same records, for tests and timing
  // With measure: also the first-order intensity statistics (K11, nm03/measure.h IntensityStats).
  bool measure_intensity = false;
  // With measure: also the grey-level co-occurrence matrix at `texture_levels` (2 … 64) grey levels over
  // the thirteen forward directions (K12, nm03/measure.h TextureGlcm).
  bool measure_texture = false;
  int texture_levels = 32;
  // ≥ 0: the dilation is the margin of `dilate_um` micrometres around the region (K16, nm03/volume_distance.h:
  // { p : D_region(p) ≤ dilate_um² } at `spacing_um`) instead of the cube / ball of dilation_size index steps,
  // inside kernels_s where the dilation is. −1 = off: nothing of K16 is touched.
  int64_t dilate_um = -1;
  // With measure: also the thickness of the dilated volume (K16, VolumeThickness) at `spacing_um`, after K12's
  // launches, inside measure_s.
  bool measure_thickness = false;
  // Not null: also compare the dilated volume with this reference mask of the same shape (K17,
  // nm03/volume_compare.h VolumeCompare) at `spacing_um`, after every measure launch. Needs no `measure`.
  const VolumeReference* compare = nullptr;
  // N > 0 (needs `compare`): also the lesion-wise comparison of the same two masks (K18,
  // nm03/volume_compare_lesions.h) with N reported lesions per side, at `measure_connectivity`, after K17's
  // launches on the same stream. 0 = off.
  int compare_lesions = 0;
};

// Runs the 3D pipeline on `device`; copies masks back when `want_masks`. A VolumeRunner keeps
// its device buffers, stream and events between runs (rebuilt when the volume shape changes);
// run_volume() is the one-shot form.
class VolumeRunner {
 public:
  explicit VolumeRunner(int device);
  ~VolumeRunner();
  VolumeRunner(const VolumeRunner&) = delete;
  VolumeRunner& operator=(const VolumeRunner&) = delete;
  // With p.measure the K8 kernels run after the segmentation (first use loads their code object and
  // allocates their scratch, kept like the other buffers); without it nothing of K8 is touched. The
  // same holds for p.measure_lesions and K10, for p.measure_intensity and K11 (after K8's last launch)
  // and for p.measure_texture and K12 (after K11's), and for p.measure_diameters and K13 (directly after
  // K10's launches; its work buffer is sized by the N asked for and regrown when a later run asks for more).
  // p.dilate_um ≥ 0 and p.measure_thickness share K16: its code object and its scratch (2 + 8 bytes per
  // voxel) come with the first run that asks for either and are kept and rebuilt with the volume shape. All
  // argument checks, the extent rule of nm03/volume_distance.h included, run before the run's first launch.
  // p.compare: K17's code object (and K16's, whose map it uses), its work buffer (18 bytes per voxel), the
  // reference's device words with their pinned staging, the pinned record and two events come with the first
  // run that asks for it and are kept and rebuilt with the volume shape; its launches follow every measure
  // launch. A reference without a buffer or of another shape and the extent rule throw std::invalid_argument
  // before the run's first launch.
  // p.compare_lesions: K18's code object, its work buffer (16 bytes per slot of K8's layout), the pinned record and
  // two events come with the first run that asks for it and are kept and rebuilt with the volume shape; its ten
  // launches follow K17's on the masks K17 already has on the device. Without `compare`, outside 1 … 64, with a
  // connectivity other than 6 / 26 or on a volume K8 could not label it throws std::invalid_argument before the
  // run's first launch.
  VolumeResult run(const VolumeInput& v, const VolumeParams& p, bool want_masks);
  // After run() on the same volume: the 2·d exported JPEG files of the 3D cohort mode, in plane
  // order (original, processed), rendered and encoded on the GPU (K3/K4) from the volume still on
  // the device — byte-identical to the golden host renderer + encoder.
  std::vector<std::vector<uint8_t>> export_jpegs(const VolumeInput& v, const VolumeParams& p, const RenderParams& rp,
                                                 struct VolumeExportStats* stats = nullptr);
  // After run() on the same volume (--volume-views): the six views through `at` from the volume and the
  // dilated bit planes still on the device (K14), each rendered into the rp canvas at the view's own
  // spacing with the renderer border of its own 2D image and encoded by K4 — byte-identical to
  // golden::volume_view_jpegs of golden::volume_views. The first call loads K14's code object and
  // allocates the view buffers, kept like the others and rebuilt with the volume shape; without a call
  // nothing of K14 is touched. Throws std::invalid_argument for a point outside the volume.
  // `want_planes`: also copy the sample and mask planes back.
  VolumeViewsExport export_views(const VolumeInput& v, const VolumeParams& p, const RenderParams& rp, const ViewsAt& at,
                                 bool want_planes = false, struct VolumeExportStats* stats = nullptr);
  // After run() on the same volume (--volume-mesh): the surface mesh of nm03/volume_mesh.h from the dilated
  // bit planes still on the device (K15), equal to golden::volume_mesh of the dilated mask at the volume's
  // spacing. The first call loads K15's code object and allocates its work buffer, kept like the others and
  // rebuilt with the volume shape; the result buffer is kept and regrown. Without a call nothing of K15 is
  // touched. One host round trip: the totals come back, the sizes are checked (vertices and 2 · quads below
  // 2^31, 12 · V + 16 · Q ≤ max_bytes; std::runtime_error naming V, Q and the cap, nothing emitted), then
  // positions and quads are written and copied back with one copy each. A volume left by run_slab is
  // refused. `scan_block`: lattice words per block of the prefix scan (0 = default).
  VolumeMesh export_mesh(const VolumeInput& v, const VolumeParams& p, int placement = kMeshCorner,
                         uint64_t max_bytes = mesh::kDefaultMaxMb << 20, int scan_block = 0);
  // One rank's z-slab of a `depth`-deep volume (volume_slabs.h): `slab` holds planes
  // [z0, z0 + slab.d); seeds (p.seeds, or the reference pattern on plane depth / 2) are in volume
  // coordinates. Preprocesses the slab's planes, runs the global region-growing fixpoint and the
  // halo cube dilation with the other ranks of `comm` (collective), leaving the slab on the device:
  // export_jpegs(slab, ...) then exports its planes. Masks (when requested) are the slab's.
  // p.measure, p.measure_lesions, p.measure_diameters, p.measure_intensity or p.measure_texture throws std::invalid_argument: components that cross slabs would
  // need a collective. p.dilate_um ≥ 0 and p.measure_thickness throw it too: a margin across slabs needs a
  // halo of its reach. p.compare throws it as well: the surface distances of a slab are not those of the volume;
  // so does p.compare_lesions (lesions that cross slabs).
  VolumeResult run_slab(Comm& comm, const VolumeInput& slab, int z0, int depth, const VolumeParams& p, bool want_masks,
                        struct SlabStats* stats = nullptr);

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};
VolumeResult run_volume(const VolumeInput& v, const VolumeParams& p, int device, bool want_masks);

namespace app {
int run_volume_cohort(const AppConfig& cfg);
}

}  // namespace nm03
