// nm03/golden.h — single-threaded CPU golden model of every pipeline stage (SURVEY §1.2 L1',
// App. A). It is the test oracle for the HIP kernels and the `--cpu` plumbing path of
// test_pipeline (BASELINE config 1). It is NOT a backend: the engine never falls back to it.
//
// Stage ↔ reference call site:
//   norm_clip        IntensityNormalization + IntensityClipping  main_sequential.cpp:195-202
//   median           VectorMedianFilter(7)                       main_sequential.cpp:204-206
//   sharpen          ImageSharpening(2.0, 0.5, 9)                main_sequential.cpp:208-210
//   region_grow      SeededRegionGrowing(0.74, 0.91, seeds)      main_sequential.cpp:232-243
//   dilate / erode   ImageCaster(UINT8) + Dilation(3) / Erosion(3) main_sequential.cpp:246-252
//   render_*         ImageRenderer / SegmentationRenderer / RenderToImage(512²)
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/common.h"
#include "nm03/measure.h"
#include "nm03/params.h"
#include "nm03/pixel_math.h"

namespace nm03 {
struct VolumeInput;  // nm03/volume.h
}

namespace nm03::golden {

struct SliceInput {
  int w = 0, h = 0;
  PixelType type = kU16;
  int stored_bits = 16;
  float slope = 1.f, intercept = 0.f;
  float spacing_x = 1.f, spacing_y = 1.f;
  std::vector<uint16_t> raw;  // raw 16-bit samples, row-major
};

// DICOM import (setLoadSeries(false)); applies the <100 guard when `min_dim` > 0.
// `frame`: dicom::select_frame policy (-1 rejects multi-frame files, k ≥ 0 imports frame k).
SliceInput load_slice(const std::string& path, int min_dim, int frame = -1);

NormClip make_normclip(const SliceInput& s, const PipelineParams& p);

std::vector<uint16_t> keys(const SliceInput& s);
std::vector<float> norm_clip(const SliceInput& s, const PipelineParams& p);
// Rescaled (modality) values used by the original-image renderer.
std::vector<float> rescaled(const SliceInput& s, const PipelineParams& p);

// Exact k×k median with clamp-to-edge (A.4).
std::vector<float> median(const std::vector<float>& img, int w, int h, int k);
std::vector<uint16_t> median_u16(const std::vector<uint16_t>& img, int w, int h, int k);
// FAST's vector-median definition (argmin_k Σ_j |w_k − w_j|, first in scan order on ties).
std::vector<float> vector_median(const std::vector<float>& img, int w, int h, int k);

// Unsharp mask with the separable contract (vertical then horizontal, taps ascending).
std::vector<float> sharpen(const std::vector<float>& img, int w, int h, float gain, float sigma, int mask);
// FAST's direct 2D mask form (for tolerance tests only).
std::vector<float> sharpen_direct(const std::vector<float>& img, int w, int h, float gain, float sigma, int mask);

std::vector<uint8_t> band(const std::vector<float>& s, float lo, float hi);
// BinaryThresholding (lo ≤ x ≤ hi → 1): the band test as a standalone op (k6_threshold.hip).
inline std::vector<uint8_t> binary_threshold(const std::vector<float>& s, float lo, float hi) { return band(s, lo, hi); }

// Seeded region growing: pixels connected (4 or 8) to an in-band seed through in-band pixels.
std::vector<uint8_t> region_grow(const std::vector<uint8_t>& band, int w, int h, const std::vector<Seed>& seeds,
                                 int connectivity);
// Square structuring element of odd `size`, out-of-image samples ignored (A.7).
// `disc`: the digital disc of radius size/2 (PipelineParams::se_shape) instead of the square.
std::vector<uint8_t> dilate(const std::vector<uint8_t>& m, int w, int h, int size, bool disc = false);
std::vector<uint8_t> erode(const std::vector<uint8_t>& m, int w, int h, int size, bool disc = false);
// SegmentationRenderer border: label pixels with a 0 within Chebyshev radius r (image space).
std::vector<uint8_t> border(const std::vector<uint8_t>& m, int w, int h, int radius);

// 3D variants (BASELINE config 5): 6/26-connected region growing, cube dilation.
std::vector<uint8_t> region_grow3d(const std::vector<uint8_t>& band, int w, int h, int d,
                                   const std::vector<Seed>& seeds, int connectivity);
// `ball`: the digital ball of radius size/2 instead of the size³ cube.
std::vector<uint8_t> dilate3d(const std::vector<uint8_t>& m, int w, int h, int d, int size, bool ball = false);

// Renderers (A.9) onto an out_w×out_h black canvas.
// `nearest`: RenderParams::filter == kFilterNearest (the source pixel under each canvas pixel's centre).
std::vector<uint8_t> render_gray(const std::vector<float>& values, const RenderGeom& g, float lo, float hi,
                                 bool nearest = false);
std::vector<uint8_t> render_labels(const std::vector<uint8_t>& label, const std::vector<uint8_t>& border_mask,
                                   const RenderGeom& g, uint8_t fill, uint8_t border_value);

// Overlay (RenderParams::overlay): the gray render with the label colour blended over it, interleaved
// RGB [out_h, out_w, 3]. Per pixel the opacity is `border_a` where the border bit is set, else `fill_a`
// where the label bit is set, else 0 (labels sampled nearest, exactly render_labels); each channel is
// overlay_blend(gray, color[c], a) (pixel_math.h). Pixels outside the image footprint stay black.
std::vector<uint8_t> render_overlay(const std::vector<float>& values, const std::vector<uint8_t>& label,
                                    const std::vector<uint8_t>& border_mask, const RenderGeom& g, float lo, float hi,
                                    bool nearest, uint8_t fill_a, uint8_t border_a, const uint8_t* color);

// Measurements of a slice (PipelineParams::measure, nm03/measure.h): the record on the `dilated` plane
// plus popcount(`region`), intensities from s.raw as stored_sample gives them. Flood-fill labelling;
// holes by labelling the complement of the padded mask at the dual connectivity.
SliceMeasure measure(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const SliceInput& s,
                     int connectivity);
// The sidecar text of a record for slice `s` under `p` (measure::to_json with the slice's fields).
std::string measure_json(const SliceMeasure& m, const SliceInput& s, const PipelineParams& p);

// Bidimensional diameters of the lesion (PipelineParams::measure_diameters, nm03/measure.h
// SliceDiameters) of a w × h mask (0/1 per pixel). Shares nothing with the K9 kernel's method: flood
// fill in raster order (the first component of the largest area is the lesion), the top and bottom
// lesion pixel of every COLUMN as candidates, plain double loops over them in (y, x) order.
SliceDiameters measure_diameters(const std::vector<uint8_t>& dilated, int connectivity, int w, int h);
// The sidecar text of a record pair (measure::to_json with the diameter keys).
std::string measure_json(const SliceMeasure& m, const SliceDiameters& d, const SliceInput& s, const PipelineParams& p);
// The sidecar text the --cpu paths write for slice `s`: measure() and, with p.measure_diameters,
// measure_diameters() at p.measure_connectivity, through the matching measure_json; with
// p.measure_intensity also measure_intensity(), its keys after all the others; with p.measure_texture
// also measure_texture() at p.texture_levels, its keys after those.
std::string measure_sidecar(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const SliceInput& s,
                            const PipelineParams& p);

// First-order intensity statistics (nm03/measure.h IntensityStats) of the stored samples under
// `dilated` (0/1 per pixel, h × w; the overload below: per voxel, d planes of h × w). The oracle of the
// K11 kernels: it collects the samples, sorts them and indexes at rank − 1, and sums the squares — no
// histogram; it shares only stored_sample and the rank formula with the kernels.
IntensityStats measure_intensity(const std::vector<uint8_t>& dilated, const SliceInput& s);
IntensityStats measure_intensity(const std::vector<uint8_t>& dilated, const VolumeInput& v);
// The volume sidecar text with the intensity keys (the matching measure::volume_to_json overloads);
// `lesions`: null without --measure-volume-lesions.
std::string measure_volume_json(const VolumeMeasure& m, const IntensityStats& st, const std::vector<VolumeLesion>* lesions,
                                int max_lesions, const VolumeInput& v, bool apply_rescale, int connectivity);

// The grey-level co-occurrence matrix (nm03/texture_core.h, nm03/measure.h TextureGlcm) of the stored
// samples under `dilated` (0/1 per pixel, h × w; the overload below: per voxel, d planes of h × w) at
// `levels` grey levels. The oracle of the K12 kernels: a plain loop over the voxels and the list of
// forward directions that adds to C[a][b] and C[b][a] — no words, no shifted masks, no directed counts.
// It shares only stored_sample, sample_key and tcore::level with the kernels.
measure::Glcm measure_texture(const std::vector<uint8_t>& dilated, const SliceInput& s, int levels);
measure::Glcm measure_texture(const std::vector<uint8_t>& dilated, const VolumeInput& v, int levels);
// The volume sidecar text with the texture keys (measure::volume_to_json with `tx`); `st`, `lesions`:
// null without --measure-intensity / --measure-volume-lesions.
std::string measure_volume_json(const VolumeMeasure& m, const IntensityStats* st, const std::vector<VolumeLesion>* lesions,
                                int max_lesions, const measure::Glcm& tx, const VolumeInput& v, bool apply_rescale,
                                int connectivity);

// Measurements of a volume (VolumeParams::measure, nm03/measure.h VolumeMeasure): the record on the
// `dilated` volume plus popcount(`region`) (0/1 per voxel, d planes of h × w), intensities from v.raw.
// Plain per-voxel code that shares nothing with the K8 kernels' word arithmetic: components by flood
// fill at `connectivity` (6 | 26), cavities by labelling the complement of the 1-voxel-padded mask at
// the dual connectivity, the Euler number by per-voxel loops over the padded array.
VolumeMeasure measure_volume(const std::vector<uint8_t>& dilated, const std::vector<uint8_t>& region, const VolumeInput& v,
                             int connectivity);
// The sidecar text of a record for volume `v` (measure::volume_to_json with the volume's fields).
std::string measure_volume_json(const VolumeMeasure& m, const VolumeInput& v, bool apply_rescale, int connectivity);
// The `max_lesions` (1 … kMaxVolumeLesions) largest components of `dilated` at `connectivity`
// (VolumeParams::measure_lesions, nm03/measure.h VolumeLesion), largest first; a tie goes to the
// component whose first voxel in raster order comes first. Independent of the K10 kernels: a flood
// fill per component with per-voxel statistics and face loops, then a sort.
std::vector<VolumeLesion> measure_volume_lesions(const std::vector<uint8_t>& dilated, const VolumeInput& v,
                                                 int connectivity, int max_lesions);
// The sidecar text with the lesion keys (the matching measure::volume_to_json overload).
std::string measure_volume_json(const VolumeMeasure& m, const std::vector<VolumeLesion>& lesions, int max_lesions,
                                const VolumeInput& v, bool apply_rescale, int connectivity);
// The lengths (nm03/measure.h VolumeLesionDiameters) of the same lesions in the same order, for a
// d × h × w mask and the spacing `um` in integer micrometres (x, y, z). Independent of the K13 kernels:
// a flood fill per component, then plain loops over the pairs of its voxels with an open 6-face (of all
// its voxels when they are few) — not the kernels' row extremes.
std::vector<VolumeLesionDiameters> measure_volume_diameters(const std::vector<uint8_t>& dilated, int w, int h, int d,
                                                            int connectivity, int max_lesions, const uint32_t um[3]);

struct SliceResult {
  std::vector<float> clipped, median, sharpened;
  std::vector<uint8_t> band, region, eroded, dilated;
  float window_lo = 0, window_hi = 0;  // original render window (rescaled min/max)
};

SliceResult run(const SliceInput& s, const PipelineParams& p, bool with_erosion);

// Render + JPEG of the two exported images of seq/par (original, processed).
struct SliceJpegs {
  std::vector<uint8_t> original, processed;
  // RenderParams::overlay only: the RGB canvas (original + dilated mask) and its JPEG file.
  std::vector<uint8_t> overlay_canvas, overlay;
};
SliceJpegs export_jpegs(const SliceInput& s, const SliceResult& r, const PipelineParams& p, const RenderParams& rp);

// test_pipeline's five stage images (test_pipeline.cpp:164-179): original, preprocessed,
// segmentation, erosion, dilation — canvases and their JPEG files. With RenderParams::overlay a
// sixth entry follows: the RGB overlay canvas (original + dilated mask) and its colour JPEG.
struct StageImages {
  std::vector<std::vector<uint8_t>> canvases, jpegs;
};
// `stages` (optional) receives the intermediate arrays (for --dump-mhd).
StageImages test_pipeline_images(const SliceInput& s, const PipelineParams& p, const RenderParams& rp,
                                 SliceResult* stages = nullptr);

}  // namespace nm03::golden
