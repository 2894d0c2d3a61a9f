// nm03/kernels.h — host-callable launchers of the gfx950 kernels (src/kernels/*.hip).
// All launchers are asynchronous on `stream` and allocation-free (graph-capturable).
#pragma once

#include <hip/hip_runtime_api.h>

#include <string>

#include "nm03/common.h"
#include "nm03/gpu_types.h"
#include "nm03/measure.h"
#include "nm03/pixel_math.h"
#include "nm03/volume_compare.h"
#include "nm03/volume_distance.h"
#include "nm03/volume_mesh.h"
#include "nm03/volume_views.h"

namespace nm03::gpu {

void check_hip(hipError_t e, const char* what);
void check_launch(const char* what);
// NM03_SYNC_LAUNCHES=1: synchronise after every launch (debugging; disables graph capture).
bool sync_launches();
// Profiling variant of `kernel` ("jpeg", "median") from NM03_PROFILE_VARIANT="jpeg=12,median=1"; 0 = the
// real kernel. Variants truncate the kernel for time splits; their output is invalid.
int profile_variant(const char* kernel);

// Loads the code object of every kernel translation unit (k1 median and sharpen, k2 SRG, k3 render,
// k4 JPEG, k5 volume, k6 threshold; every template instance) on the current device. HIP loads a
// translation unit's code object at the first launch of one of its kernels; preloading makes that
// happen on one thread before any launch (Engine and VolumeEngine constructors), never from a slot
// thread in the middle of a run. Fails loudly (DeviceError) when a code object does not load.
// with_volume = false leaves out k5 volume and k6 threshold, which the 2D engine never launches.
void preload_kernels(bool with_volume = true);
void preload_median();
void preload_sharpen();
void preload_srg();
void preload_render();
void preload_volume();
void preload_threshold();

// The engine's per-format normalise+clip table (n = 2^stored_bits keys from `base`), built on the
// device on `stream` with the shared pixel_math.h function.
void launch_build_norm_lut(float* out, uint32_t n, uint32_t base, uint8_t type, const NormClip& nc, hipStream_t stream);
// The first host→device copy of a process initialises the runtime's copy path (≈ 10 ms on a cold
// MI355X process, profiles/r5/cold/): one 4 MiB pinned H2D on `stream` (the SDMA path), synchronised.
void warm_copy_path(hipStream_t stream);

// K1a: k×k median of raw keys → `med` (u16 keys, same layout as raw). k ∈ {3,5,7,9}.
// Per-slice key range: with `tile_mm` (2 u32 per tile) each tile stores its (min, max) and
// launch_sharpen_band reduces them into stats (no atomics); without it, atomics on stats.
// With `blob` (engine batches) the samples are read from the uploaded blob at SliceDesc::blob_off
// (12-bit packed slices decoded on the fly) instead of `raw`, and the expanded 16-bit samples are
// written to `raw_out` at raw_off (the samples the render stage reads).
void launch_median(const uint16_t* raw, uint16_t* med, const SliceDesc* descs, const TileDesc* tiles, int ntiles,
                   int k, SliceStats* stats, hipStream_t stream, uint32_t* tile_mm = nullptr,
                   const uint16_t* blob = nullptr, uint16_t* raw_out = nullptr);

// K1b: normalise+clip of the median keys, separable Gaussian unsharp mask, SRG band test →
// `band` bitmaps (u64 words, LSB = left-most pixel). Optionally the f32 sharpened image.
// `lut` (optional): the engine's normalise+clip tables (SliceDesc::lut_off / lut_base).
void launch_sharpen_band(const uint16_t* med, uint64_t* band, float* sharpened, const SliceDesc* descs,
                         const TileDesc* tiles, int ntiles, const PipeConsts& pc, SliceStats* stats,
                         hipStream_t stream, const uint32_t* tile_mm = nullptr, const float* lut = nullptr);

// Bitmap planes produced by K2 (each null when not requested).
struct SrgOutputs {
  uint64_t* region = nullptr;
  uint64_t* dilated = nullptr;
  uint64_t* eroded = nullptr;
  uint64_t* border_region = nullptr;
  uint64_t* border_eroded = nullptr;
  uint64_t* border_dilated = nullptr;
  int32_t* iterations = nullptr;  // per-slice fixpoint iteration count (diagnostics)
  // Slices larger than kSrgMaxDim: 4 × srg_scratch_words(max_w, max_h) words per slice of device
  // scratch for the bit planes (the LDS-resident form cannot hold them).
  uint64_t* scratch = nullptr;
};
// Words per bit plane of the K2 kernel for slices up to max_w × max_h (odd row strides).
size_t srg_plane_words(int max_w, int max_h);

// K2: LDS-resident seeded region growing (bit-parallel run fills on rows and on the transposed
// bitmap until fixpoint) + dilation/erosion + renderer borders. One workgroup per slice; the four
// bit planes live in LDS for slices ≤ kSrgMaxDim, else in `out.scratch` (same code, global memory).
void launch_srg_morph(const uint64_t* band, const SliceDesc* descs, int nslices, const SeedXY* seeds,
                      const PipeConsts& pc, const SrgOutputs& out, int max_w, int max_h, hipStream_t stream);

// 3D region growing on a w×h×d bit volume (planes of h rows × ceil(w/64) words) by plane sweeps in
// ONE cooperative launch that decides convergence on the device (k5_volume.hip): no host
// synchronisation. seeds_xyz: device int32 triples. d_ctl: kSrg3dCtlWords device words; h_ctl
// (optional): pinned host words receiving them at the end of the launch — srg_volume_result(h_ctl)
// after the stream is synchronised gives the sweep count, or throws: the region is the fixpoint or
// the call fails (the sweeps are bounded by the voxel count, a true bound). Planes too large for LDS
// (a side > 512) need `scratch` of srg3d_scratch_words(w, h, d) words. reset = false continues from
// the region already in `region` (⊆ band): the z-slab decomposition (volume_slabs.h) re-grows a slab
// after neighbouring slabs contributed boundary voxels.
constexpr int kSrg3dCtlWords = 8;
size_t srg3d_scratch_words(int w, int h, int d);
void srg_volume(const uint64_t* band, uint64_t* region, int w, int h, int d, const int32_t* seeds_xyz, int nseeds,
                int connectivity, uint32_t* d_ctl, uint32_t* h_ctl, uint64_t* scratch, hipStream_t stream,
                bool reset = true);
int srg_volume_result(const uint32_t* h_ctl);
// Scratch for border_volume / dilate_volume when a plane does not fit LDS (else 0).
size_t morph3d_scratch_words(int w, int h, int d);
// Largest structuring-element size of the 3D morphology (the 2D engine's limit): the row shifts
// combine a word with one neighbour on each side, so a radius stays below 64. Sizes are odd.
constexpr int kMorph3dMaxSize = 63;
// Per-plane renderer border of a bit volume: label ∧ ¬erode_{(2r+1)²}(label) (2D, every plane).
void border_volume(const uint64_t* src, uint64_t* dst, int w, int h, int d, int radius, hipStream_t stream,
                   uint64_t* scratch = nullptr);
// Cube dilation of a bit volume (size odd), separable; `tmp` same size as the volume.
// `ball`: the digital ball of radius size/2 (one pass, dilate_ball_kernel) instead of the size³ cube.
void dilate_volume(const uint64_t* src, uint64_t* dst, uint64_t* tmp, int w, int h, int d, int size,
                   hipStream_t stream, uint64_t* scratch = nullptr, bool ball = false);
// z-slab boundary step (volume_slabs.h), one plane: add = band ∧ touch(nb) ∧ ¬region, region |= add,
// *added += popcount(add); touch = nb (6-connectivity) or its 3×3 in-plane dilation (26).
void launch_slab_seed(const uint64_t* band, uint64_t* region, const uint64_t* nb, int w, int h, bool conn26,
                      unsigned long long* added, hipStream_t stream);

// K3: render canvases (out_w×out_h u8 each).
void launch_render(const uint16_t* raw, const float* f32, const uint64_t* bits, const SliceStats* stats,
                   const RenderDesc* rd, int ncanvas, int out_w, int out_h, uint8_t* canvas, hipStream_t stream);

// K4: JPEG in one pass, workgroup per 256 luma blocks of an image: [fused 2× render or canvas
// read] → islow FDCT → reciprocal quantisation → Huffman coding → workgroup scan → bit range in
// LDS → decoupled look-back across the image (bit offset and 0xFF-stuffing count) → the stuffed
// bytes straight into `out` (host-mapped pinned memory, JpegDesc.out_off).
// out_sizes[i] = bytes, or -1 when the image exceeded its staging/out capacity (caller
// re-encodes on the CPU).
struct JpegWork {
  uint64_t* look = nullptr;      // 2 × 3 × look_cap record words, zeroed once at allocation: two
                                 // halves, each launch uses one and clears the other (launch_jpeg)
  size_t look_cap = 0;           // ≥ ncanvas × ceil(blocks / 256) workgroups
  size_t look_used = 0;          // set by launch_jpeg
  size_t look_base = 0, clear_base = 0, clear_words = 0, prev_words = 0;  // launch_jpeg's bookkeeping
  uint32_t* ticket = nullptr;    // per-image part ticket counters (≥ ncanvas; zeroed once; self-resetting)
  uint32_t* spill = nullptr;     // look_cap × 256 × 56 words: Huffman bits of very detailed blocks
};
// Fused-render inputs (needed when any JpegDesc.render ≥ 0).
struct JpegRenderSrc {
  const uint16_t* raw = nullptr;
  const float* f32 = nullptr;
  const uint64_t* bits = nullptr;
  const SliceStats* stats = nullptr;
  // Render descriptors, one per canvas: JpegDesc k's `render` is either -1 (encode canvas k from
  // `canvas`) or k itself (render descriptor k fused into the encoder). launch_jpeg checks that
  // `nrd` covers every canvas when rd is set.
  const RenderDesc* rd = nullptr;
  int nrd = 0;
};
void launch_jpeg(const uint8_t* canvas, const JpegDesc* jd, int ncanvas, int out_w, int out_h, const int32_t* div_luma,
                 JpegWork& w, uint8_t* out, int32_t* out_sizes, hipStream_t stream,
                 const JpegRenderSrc* fused = nullptr, int sampling = 0,  // jpeg::Sampling
                 bool nearest = false);  // fused gray renders use --render-filter nearest (4:2:0 only)
// Whether the fused encoder renders --render-filter nearest gray images for this layout (else callers
// render them into canvases first).
inline bool jpeg_fuses_nearest(int sampling) { return sampling == 0; }
// K4-RGB (k4_jpeg_rgb.hip): colour JPEG of interleaved RGB canvases (out_w × out_h × 3 bytes at
// JpegDesc::canvas_off of `canvas`; render and stage fields unused) → YCbCr 4:2:0 or 4:4:4 segments,
// the gray encoder's structure and `out` / `out_sizes` / capacity semantics. `w` needs look_cap ≥
// ncanvas × jpeg_rgb_parts(...) (its spill area is sized by look_cap as for launch_jpeg); it may be
// the JpegWork of launch_jpeg calls on the same stream.
size_t jpeg_rgb_parts(int out_w, int out_h, int sampling);
void launch_jpeg_rgb(const uint8_t* canvas, const JpegDesc* jd, int ncanvas, int out_w, int out_h, const int32_t* div_luma,
                     const int32_t* div_chroma, JpegWork& w, uint8_t* out, int32_t* out_sizes, hipStream_t stream,
                     int sampling = 0);
// Loads the colour encoder's code object on the current device. Not part of preload_kernels: only
// an engine with the overlay on (in its constructor) and the Python op (before its first launch)
// load it, so a default run never pays for it — and no slot thread ever loads it lazily.
void preload_jpeg_rgb();

// K3 overlay: RGB canvas i (3 · out_w · out_h bytes at rgb + i · 3 · out_w · out_h) = the gray render
// rd[gray_first + i · stride] with colour `rgb_color` (R | G << 8 | B << 16) blended over it at the
// opacity the label render rd[label_first + i · stride] gives the pixel (its border_value / fill / 0)
// — pixel_math.h overlay_blend. Any geometry; out_w a multiple of 4.
void launch_render_overlay(const uint16_t* raw, const float* f32, const uint64_t* bits, const SliceStats* stats,
                           const RenderDesc* rd, int gray_first, int label_first, int stride, int ncanvas, int out_w,
                           int out_h, uint32_t rgb_color, uint8_t* rgb, hipStream_t stream);

// K7 (k7_measure.hip): per-slice measurements of the `dilated` plane plus popcount(`region`)
// (nm03/measure.h), one workgroup per slice, slices of different sizes in one launch (SliceDesc::w, h,
// wpr, mask_off, raw_off, type, stored_bits). `raw`: the expanded 16-bit samples at raw_off. `out`:
// nslices records, written with plain vector stores (device or host-mapped memory). `scratch`: nslices ×
// measure_scratch_words(max_w, max_h) words for the labelling's parents and areas, no initialisation
// needed; max_w / max_h bound every slice of the launch (a slice that does not fit its share is not
// measured and reports components = 0xFFFFFFFF). No host round trip, no allocation.
size_t measure_scratch_words(int max_w, int max_h);
void launch_measure(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, const SliceDesc* descs, int nslices,
                    int connectivity, SliceMeasure* out, uint32_t* scratch, int max_w, int max_h, hipStream_t stream);
// Loads K7's code object on the current device. Not part of preload_kernels: only an engine with
// PipelineParams::measure (in its constructor) and the Python op (before its first launch) load it,
// so a default run never pays for it — and no slot thread ever loads it lazily.
void preload_measure();

// K9 (k9_diameters.hip): the SliceDiameters record (nm03/measure.h) of every slice's lesion, one
// workgroup per slice, launched on the stream of a launch_measure call with the same `dilated`,
// `descs`, `nslices`, `scratch`, `max_w` and `max_h`: it reads K7's labelling as that launch leaves it
// (every run start points at its root, the component's area in the slot after the root) and writes
// nothing but `out` (plain vector stores; device or host-mapped memory). A slice that K7 could not
// measure reports lesion_px = kDiametersNotMeasured. No host round trip, no allocation.
void launch_measure_diameters(const uint64_t* dilated, const SliceDesc* descs, int nslices, SliceDiameters* out,
                              const uint32_t* scratch, int max_w, int max_h, hipStream_t stream);
// Loads K9's code object on the current device: as preload_measure, only for an engine with
// PipelineParams::measure_diameters and the Python op.
void preload_measure_diameters();

// K8 (k8_volume_measure.hip): the VolumeMeasure record (nm03/measure.h) of the `dilated` bit volume
// (d planes of h rows of ceil(w / 64) words) plus popcount(`region`), the intensities from `raw`
// (plane z at raw + z · raw_plane_stride). Twelve small launches on `stream` (multi-workgroup phases
// separated by kernel boundaries; no host round trip, no allocation). `scratch`:
// volume_measure_scratch_words(w, h, d) u32, no initialisation needed; `acc`: kVolumeMeasureAccWords
// u64 of device memory; `out`: one record, written with plain vector stores (device, pinned or
// host-mapped memory). Throws DeviceError before any launch for a volume whose (w + 1)·h·d + 1 slots
// do not fit 32 bits, and for a connectivity other than 6 / 26.
using nm03::volume_measure_scratch_words;
constexpr int kVolumeMeasureAccWords = 32;
// `lesions` (optional, --measure-volume-lesions): the K10 launches below are enqueued between the two
// passes; null leaves the twelve launches as they are.
// `diameters` (optional, --measure-volume-diameters): the K13 launches follow K10's.
struct VolumeDiametersWork {
  void* work = nullptr;                  // volume_diameters_work_bytes(w, h, d, N) of device memory, no initialisation needed
  VolumeLesionDiameters* out = nullptr;  // N records (device, pinned or host-mapped memory); those past the count are zero
  uint32_t spacing_um[3] = {1000u, 1000u, 1000u};  // x, y, z in integer micrometres, each ≥ 1
  bool brute_force = false;              // compare every tile pair (the records are the same; for tests and timing)
};
struct VolumeLesionWork {
  int max_lesions = 0;            // N, 1..kMaxVolumeLesions
  void* work = nullptr;           // volume_lesions_work_bytes(w, h, d, N) of device memory, no initialisation needed
  VolumeLesion* out = nullptr;    // N records (device, pinned or host-mapped memory); those past the count are zero
  uint32_t* out_count = nullptr;  // the reported count, min(N, components)
  const VolumeDiametersWork* diameters = nullptr;  // null = off: the launch sequence stays as it is
};
void launch_volume_measure(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, size_t raw_plane_stride,
                           int w, int h, int d, uint8_t type, uint8_t stored_bits, int connectivity, uint32_t* scratch,
                           uint64_t* acc, VolumeMeasure* out, hipStream_t stream,
                           const VolumeLesionWork* lesions = nullptr);
// Loads K8's code object on the current device. Not part of preload_kernels: only a VolumeRunner's
// first measuring run (before that run's first launch, while its stream is idle) and the Python op
// (before its first launch) load it, so a run without --measure-volume never pays for it.
void preload_volume_measure();

// K10 (k10_volume_lesions.hip): the VolumeLesion records (nm03/measure.h) of the N largest components
// of the `dilated` bit volume, from K8's labelling of the mask as vm_roots_kernel leaves it in
// `scratch` (launch_volume_measure enqueues this between its two passes). Five launches on `stream`:
// init, candidates (every workgroup's N best roots), select (one workgroup), accumulate (a thread per
// word), final. No host round trip, no allocation; records and count are written with plain vector
// stores. The candidate list holds N keys per workgroup of the word grid, so it cannot overflow.
size_t volume_lesions_work_bytes(int w, int h, int d, int max_lesions);
void launch_volume_lesions(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                           uint8_t type, uint8_t stored_bits, const uint32_t* scratch, const VolumeLesionWork& lesions,
                           hipStream_t stream);
// Loads K10's code object on the current device: only a VolumeRunner's first run that asks for lesions
// and the Python op load it.
void preload_volume_lesions();

// K13 (k13_volume_diameters.hip): the VolumeLesionDiameters records (nm03/measure.h) of the lesions K10
// chose, in K10's order: the 3D major diameter, the largest axial diameter and its perpendicular in
// integer micrometres. launch_volume_measure enqueues it directly after K10 when
// VolumeLesionWork::diameters is set, before the complement pass overwrites the labelling. Seven launches
// on `stream`: init, rows (the extremes of every lesion row, a thread per word), tiles (boxes of 128
// rows), bound (one workgroup per lesion), planes (the axial bound, a wave per plane), pairs (a fixed grid
// over the tile pairs, skipping those whose boxes lie strictly below the bounds), final. It reads `scratch`, K10's chosen roots and bounding boxes
// in `lesions.work`, and writes only its own work buffer and records (plain vector stores). No host
// round trip, no allocation. Throws DeviceError before any launch when a (dim − 1) · spacing_um reaches
// 2^31, naming the product. The work buffer is 8 · N · h · d bytes for the row table plus the tile boxes
// and the partial slots.
size_t volume_diameters_work_bytes(int w, int h, int d, int max_lesions);
// The checks of launch_volume_diameters alone (launch_volume_measure makes them before its first launch).
void validate_volume_diameters(const uint64_t* dilated, int w, int h, int d, const uint32_t* scratch,
                               const VolumeLesionWork& lesions);
void launch_volume_diameters(const uint64_t* dilated, int w, int h, int d, const uint32_t* scratch,
                             const VolumeLesionWork& lesions, hipStream_t stream);
// Loads K13's code object on the current device: only a run that asks for diameters and the Python op load it.
void preload_volume_diameters();

// K11 (k11_intensity.hip), 2D: the IntensityStats record (nm03/measure.h) of the samples under every
// slice's `dilated` plane, one workgroup per slice, slices of different sizes in one launch
// (SliceDesc::w, h, wpr, mask_off, raw_off, type, stored_bits), a two-pass radix select in LDS. It reads
// what K7 reads and writes nothing but `out` (nslices records, plain vector stores; device or
// host-mapped memory). No global scratch, so every slice is measured; no host round trip, no allocation.
void launch_measure_intensity(const uint64_t* dilated, const uint16_t* raw, const SliceDesc* descs, int nslices,
                              IntensityStats* out, hipStream_t stream);
// K11, 3D: the record of the samples under the `dilated` bit volume (d planes of h rows of ceil(w / 64)
// words; plane z of the samples at raw + z · raw_plane_stride). Five small launches on `stream`
// (init, high-byte histogram, select, low-byte histogram, final) separated by kernel boundaries; no host
// round trip, no allocation. `acc`: kVolumeIntensityAccBytes of device memory, no initialisation needed;
// `out`: one record, written with plain vector stores (device, pinned or host-mapped memory). Throws
// DeviceError before any launch for a volume that launch_volume_measure refuses.
constexpr size_t kVolumeIntensityAccBytes = 8192;
void launch_volume_intensity(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                             uint8_t type, uint8_t stored_bits, void* acc, IntensityStats* out, hipStream_t stream);
// Load K11's code object on the current device. Not part of preload_kernels: only an engine or a
// VolumeRunner built with the feature on and the Python ops (before their first launch) load it.
void preload_measure_intensity();
void preload_volume_intensity();

// K12 (k12_texture.hip), 2D: the TextureGlcm record (nm03/measure.h: a 64-byte header, then the
// levels × levels co-occurrence matrix as uint32) of the samples under every slice's `dilated` plane, one
// workgroup per slice, slices of different sizes in one launch (SliceDesc as for K11). `slots` null:
// every slice at `levels` grey levels (2 … 64), record i at out + i · glcm_record_bytes(levels). `slots`
// given (nslices of them, device memory): slice i at slots[i].levels, its record at 32-bit word
// slots[i].word_off of `out`; `levels` is not used. It reads what K11 reads and writes nothing but `out`
// (plain vector stores of 32-bit words; device or host-mapped memory, 4-byte aligned). No global scratch,
// no host round trip, no allocation.
struct TextureSlot {
  uint32_t levels;
  uint32_t word_off;
};
void launch_measure_texture(const uint64_t* dilated, const uint16_t* raw, const SliceDesc* descs, int nslices,
                            const TextureSlot* slots, int levels, void* out, hipStream_t stream);
// K12, 3D: the record of the samples under the `dilated` bit volume (laid out as for
// launch_volume_intensity), thirteen forward directions. Four small launches on `stream` (init, range,
// histogram, final) separated by kernel boundaries; no host round trip, no allocation. `acc`:
// kVolumeTextureAccBytes of device memory, no initialisation needed; `out`: glcm_record_bytes(levels),
// written with plain vector stores (device, pinned or host-mapped memory). Throws DeviceError before any
// launch for a volume that launch_volume_measure refuses.
constexpr size_t kVolumeTextureAccBytes = 16 * 16384 + 64;
void launch_volume_texture(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                           uint8_t type, uint8_t stored_bits, int levels, void* acc, void* out, hipStream_t stream);
// Load K12's code object on the current device. Not part of preload_kernels: only an engine or a
// VolumeRunner built with the feature on and the Python ops (before their first launch) load it.
void preload_measure_texture();
void preload_volume_texture();

// K14 (k14_volume_views.hip): the six views of nm03/volume_views.h from the samples `raw` (plane z at raw
// + z · raw_plane_stride) and the `dilated` bit volume (d planes of h rows of ceil(w / 64) words), in the
// buffers K3 / K4 render from. Five launches on `stream`, separated by kernel boundaries: init (zero the
// projection scratch and the shadows), project (ONE read of the volume and of the bit planes: a workgroup
// owns 128 columns × 16 rows × 8 planes and combines its partial maxima / ORs with integer
// atomicMax / atomicOr where more than one workgroup contributes), point (one workgroup: the box of the
// mask from the shadows, then P), extract (the three planes through P, the projections narrowed to
// samples, every gray view's key min / max by atomicMin / atomicMax), count (every mask's popcount by one
// workgroup each). No grid barrier, flag, spin, host round trip or allocation; the result does not depend on the
// order in which workgroups run.
struct VolumeViewsLayout {
  int w = 0, h = 0, d = 0;
  int vw[kVolumeViewCount], vh[kVolumeViewCount], wpr[kVolumeViewCount];  // view i: width, height, mask words per row
  uint32_t sample_off[kVolumeViewCount];  // u16 elements into `samples` (multiples of 8)
  // u64 words into `bits`: the mask of view i; its renderer border goes border_off words further. Views of
  // one size are neighbours (0, 3 | 1, 4 | 2, 5), so border_volume takes each pair as a two-plane volume.
  uint32_t mask_off[kVolumeViewCount];
  uint32_t border_off = 0;        // = the words of all six masks
  uint32_t proj_off[3] = {0, 0, 0};  // u32 elements into `proj`: the projection along z, y, x
  size_t samples = 0, bit_words = 0, proj = 0;  // buffer sizes: u16 elements, u64 words (masks + borders), u32 elements
};
// Throws DeviceError for an empty volume or one whose views do not fit 32-bit offsets.
VolumeViewsLayout volume_views_layout(int w, int h, int d);
// What the kernels leave for the host, copied back once: P, the box and the per-view integers.
struct VolumeViewsHead {
  int32_t at[3];
  int32_t has_box;
  int32_t box[6];
  uint32_t mask_px[kVolumeViewCount];
  SliceStats stats[kVolumeViewCount];  // key_min / key_max of every gray view (K3's window); s_* unused
};
// `inverted`: the smallest key wins a projection. `at` must have passed views::at_error. `samples`,
// `bits`, `proj`: L.samples u16, L.bit_words u64, L.proj u32 of device memory, no initialisation needed;
// `head`: device memory. Throws DeviceError before any launch for a null buffer, stored bits outside
// 1..16, a plane stride below w · h or a volume of more than 2^32 − 1 samples.
void launch_volume_views(const uint16_t* raw, size_t raw_plane_stride, const uint64_t* dilated, uint8_t type,
                         uint8_t stored_bits, bool inverted, const ViewsAt& at, const VolumeViewsLayout& L, uint16_t* samples,
                         uint64_t* bits, uint32_t* proj, VolumeViewsHead* head, hipStream_t stream);
// Loads K14's code object on the current device: only a VolumeRunner's first export_views and the Python
// op load it.
void preload_volume_views();

// K15 (k15_volume_mesh.hip): the surface mesh of nm03/volume_mesh.h from the `dilated` bit volume (d planes of
// h rows of ceil(w / 64) words), a thread per u64 word of the lattice. Two halves around the one host round
// trip. launch_volume_mesh: classify (mixed and face words with their popcounts, the voxel count), then the
// exclusive prefix of the four count streams in raster order — block totals, one workgroup over the totals,
// downsweep, `scan_block` lattice words per block — and the head (four totals, voxel count) copied to the
// pinned `h_head`. After the stream is synchronised the host sizes the result (mesh::size_error) and
// launch_volume_mesh_emit writes the positions (3 · V floats) and the quads (4 · Q indices, x then y then z)
// with plain vector stores. Separate launches; no cooperative launch, grid barrier, flag, look-back or spin.
// `work`: volume_mesh_work_bytes of device memory, no initialisation needed, kept between the two halves.
struct VolumeMeshHead {
  uint64_t total[4];  // vertices, x-quads, y-quads, z-quads
  uint64_t voxels;
};
constexpr int kVolumeMeshScanBlock = mesh::kScanBlock;        // the default
constexpr int kVolumeMeshMinScanBlock = mesh::kMinScanBlock;  // tests force many blocks on a small volume
constexpr int kVolumeMeshMaxScanBlock = mesh::kMaxScanBlock;
struct VolumeMeshLayout {
  int w = 0, h = 0, d = 0;
  int lw = 0;           // lattice words per row, ceil((w + 1) / 64)
  uint32_t words = 0;   // lattice words, lw · (h + 1) · (d + 1) < 2^31
  uint32_t scan_block = 0, blocks = 0;
  size_t off_head = 0, off_bits = 0, off_counts = 0, off_blocks = 0;  // byte offsets into `work`
  size_t bytes = 0;     // 48 bytes per lattice word, 16 per block, the head
};
// scan_block 0 = the default. Throws DeviceError for an empty volume, a lattice of 2^31 words or more and a
// scan block outside kVolumeMeshMinScanBlock .. kVolumeMeshMaxScanBlock.
VolumeMeshLayout volume_mesh_layout(int w, int h, int d, int scan_block = 0);
size_t volume_mesh_work_bytes(int w, int h, int d, int scan_block = 0);
void launch_volume_mesh(const uint64_t* dilated, const VolumeMeshLayout& L, void* work, VolumeMeshHead* h_head,
                        hipStream_t stream);
// `totals`: the head launch_volume_mesh left, read after the stream was synchronised; `positions` / `quads`
// hold at least its 3 · V floats and 4 · Q indices (16-byte aligned). Throws DeviceError before any launch
// when V or 2 · Q reaches 2^31. An empty mask launches nothing.
void launch_volume_mesh_emit(const uint64_t* dilated, const VolumeMeshLayout& L, const void* work, const VolumeMeshHead& totals,
                             int placement, float sx, float sy, float sz, float* positions, uint32_t* quads, hipStream_t stream);
// Loads K15's code object on the current device: only a VolumeRunner's first export_mesh and the Python op
// load it.
void preload_volume_mesh();

// K16 (k16_volume_distance.hip): the exact Euclidean distance map of nm03/volume_distance.h from a bit volume
// (d planes of h rows of ceil(w / 64) words), a wave per u64 word, lane = voxel. Three separable passes as
// separate launches on `stream` — rows (u16 index distances), cols and planes (the outward search of
// nm03/volume_distance_core.h on i64 values) — and the last pass ends in one of three ways:
//   launch_volume_distance   stores the i64 map (w · h · d values, raster z, y, x; device memory); cap_um < 0 =
//                            no cap, `to_background` measures to the zero voxels of the frame
//   launch_volume_margin     stores the bits of { D_region ≤ radius_um² } into `dilated` (the layout of `region`,
//                            every word written, bits past the width zero); no map is materialised
//   launch_volume_thickness  keeps the best (value, smallest position) over the mask voxels in a slot per
//                            workgroup, then ONE workgroup writes the 32-byte record to `out` (device, pinned or
//                            host-mapped memory) with plain vector stores
// No cooperative launch, grid barrier, flag, look-back, spin, atomic, host round trip or allocation. `work`:
// volume_distance_work_bytes of device memory (2 + 8 bytes per voxel and 16 KiB of slots), no initialisation
// needed. Each throws DeviceError before any launch for a null buffer, a spacing below 1, a negative radius and
// the extent rule (measure::volume_distance_extent_error, naming the sum).
constexpr int kVolumeDistanceWordsPerBlock = 4;
struct VolumeDistanceLayout {
  int w = 0, h = 0, d = 0, wpr = 0;
  uint32_t words = 0, blocks = 0;                     // wpr · h · d < 2^31; workgroups of every launch
  size_t off_rows = 0, off_cols = 0, off_slots = 0;  // byte offsets into `work`
  size_t bytes = 0;
};
// Throws DeviceError for an empty volume, a width above 65535 and a volume of 2^31 words or more.
VolumeDistanceLayout volume_distance_layout(int w, int h, int d);
size_t volume_distance_work_bytes(int w, int h, int d);
void launch_volume_distance(const uint64_t* bits, const VolumeDistanceLayout& L, const uint32_t um[3], bool to_background,
                            int64_t cap_um, void* work, int64_t* out, hipStream_t stream);
void launch_volume_margin(const uint64_t* region, const VolumeDistanceLayout& L, const uint32_t um[3], int64_t radius_um, void* work,
                          uint64_t* dilated, hipStream_t stream);
void launch_volume_thickness(const uint64_t* mask, const VolumeDistanceLayout& L, const uint32_t um[3], void* work,
                             VolumeThickness* out, hipStream_t stream);
// Loads K16's code object on the current device: only a VolumeRunner's first run that asks for a margin in
// millimetres or the thickness, and the Python ops, load it.
void preload_volume_distance();

// K17 (k17_volume_compare.hip): the comparison of nm03/volume_compare.h between two bit volumes `a` and `b` of
// one frame (d planes of h rows of ceil(w / 64) words, bits past the width tolerated). Twenty launches on
// `stream`: init, the surfaces with the five counts, then per direction K16's launch_volume_distance of the other
// surface (no cap), the sampling pass, two select / histogram pairs of the 11 + 11 + 10 bit radix select and the
// launch that writes the directed record to `out` (device, pinned or host-mapped memory) with plain vector
// stores. No cooperative launch, grid barrier, flag, look-back, spin, host round trip or allocation. `work`:
// volume_compare_work_bytes of device memory (two surface volumes, 48 KiB of accumulators, 16 KiB of slots, the
// i64 map and K16's own scratch: 18 bytes per voxel in all), no initialisation needed. `max_blocks`: a lower cap
// on the workgroups of the sampling and histogram launches (0 = the default 1024); the record does not depend on
// it. Throws DeviceError before any launch for a null buffer, a spacing below 1 and the extent rule.
struct VolumeCompareLayout {
  VolumeDistanceLayout dist;  // K16's layout of the same frame
  uint32_t blocks = 0;        // 256-word blocks
  size_t off_surface_a = 0, off_surface_b = 0, off_acc = 0, off_slots = 0, off_map = 0, off_dist = 0;  // byte offsets into `work`
  size_t bytes = 0;
};
// Throws DeviceError for what volume_distance_layout refuses and for a volume of 2^32 voxels or more.
VolumeCompareLayout volume_compare_layout(int w, int h, int d);
size_t volume_compare_work_bytes(int w, int h, int d);
void launch_volume_compare(const uint64_t* a, const uint64_t* b, const VolumeCompareLayout& L, const uint32_t um[3], void* work,
                           VolumeCompare* out, hipStream_t stream, int max_blocks = 0);
// Loads K17's code object on the current device: only a VolumeRunner's first run that asks for a comparison, and
// the Python op, load it. K16's is loaded separately (preload_volume_distance).
void preload_volume_compare();

// K18 (k18_volume_compare_lesions.hip): the lesion-wise comparison of nm03/volume_compare_lesions.h between two bit
// volumes `a` and `b` of one frame (d planes of h rows of ceil(w / 64) words, bits past the width tolerated). Ten
// launches on `stream`: init, then for both masks in one grid each K8's runs, unions, runs pointed at their roots
// (with the side data of the roots set), areas and K10's candidates, the selection (a workgroup per side), the
// join of the two labellings, the count of lesions / hit / multi and the launch that writes the record to `out`
// (volume_compare_lesions_record_bytes(max_lesions) of device, pinned or host-mapped memory) with plain vector
// stores. No cooperative launch, grid barrier, flag, look-back, spin, host round trip or allocation. `work`:
// volume_compare_lesions_work_bytes of device memory (16 bytes per slot of K8's layout, a 35 KiB control block and
// the candidate lists), no initialisation needed; 0 for arguments the launcher refuses. `max_blocks`: a lower cap on
// the workgroups of the join (0 = the default 1024); the record does not depend on it. Throws DeviceError before any
// launch for a null buffer, max_lesions outside 1 … kMaxVolumeLesions, a connectivity other than 6 / 26 and a volume
// whose (w + 1)·h·d + 1 slots do not fit 32 bits.
size_t volume_compare_lesions_work_bytes(int w, int h, int d, int max_lesions);
void launch_volume_compare_lesions(const uint64_t* a, const uint64_t* b, int w, int h, int d, int max_lesions, int connectivity, void* work,
                                   void* out, hipStream_t stream, int max_blocks = 0);
// Loads K18's code object on the current device: only a VolumeRunner's first run that asks for the lesion-wise
// comparison, and the Python op, load it.
void preload_volume_compare_lesions();

// K6: binary threshold lo ≤ x ≤ hi → u8 0/1 (in 16-byte aligned, out 4-byte aligned).
void launch_threshold(const float* in, uint8_t* out, size_t n, float lo, float hi, hipStream_t stream);

// True when RenderDesc r is an exact 2× fit onto the canvas (the fused fast path applies).
bool render_is_exact_2x(const RenderDesc& r, int out_w, int out_h);

// Upload the 64 islow divisors (8·Q, natural order) for `quality` into a device buffer.
void jpeg_divisors(int quality, int32_t* host_out64);

}  // namespace nm03::gpu
