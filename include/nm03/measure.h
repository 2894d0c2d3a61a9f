// nm03/measure.h — per-slice lesion measurements (--measure): the record the K7 kernel writes, the
// bit-quad arithmetic shared by the kernel and the host (as pixel_math.h shares the pixel
// arithmetic), and the one function that turns a record into the sidecar text.
//
// Everything in the record is an exact integer, measured on the DILATED plane (the mask that
// `_processed.jpg` shows) plus the popcount of the region plane; the derived doubles (mm², centroid,
// mean) exist only in to_json, which the engine, run_single, the --cpu paths and the Python binding
// all call, so they cannot differ between the GPU path and the golden path.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/common.h"

namespace nm03 {

struct alignas(64) SliceMeasure {
  uint32_t area_px;          // popcount(dilated)
  uint32_t region_px;        // popcount(region)
  int32_t bbox[4];           // x0, y0, x1, y1 inclusive; all −1 for an empty mask
  uint64_t sum_x, sum_y;     // coordinate sums over mask pixels (centroid = sum / area, on the host)
  uint32_t perimeter_edges;  // 4-neighbour pixel edges between a mask pixel and a non-mask pixel or the frame
  uint32_t components;       // connected components at the measurement connectivity (4 | 8)
  uint32_t largest_px;       // area of the largest component
  uint32_t holes;            // background components that do not reach the frame, at the dual connectivity
  int64_t raw_sum;           // over the stored sample values under the mask (0 / 0 / 0 when empty)
  int32_t raw_min, raw_max;
};
static_assert(sizeof(SliceMeasure) == 128, "SliceMeasure layout");

// Bidimensional diameters of the lesion (--measure-diameters): the record the K9 kernel writes for one
// slice. The lesion is the largest connected component of the dilated mask at the measurement
// connectivity (a tie in area goes to the component whose first pixel in raster order comes first).
// Everything is an exact integer in pixel index space, centre to centre:
//   major: the pair (a, b) of lesion pixels that maximises major_px2 = (xb − xa)² + (yb − ya)²; a does
//          not follow b in (y, x) order, a tie goes to the lexicographically smallest (ya, xa, yb, xb).
//   perp:  with (dx, dy) = b − a every lesion pixel is projected on n = (−dy, dx): p = −dy·x + dx·y.
//          perp_extent = max − min of p (the caliper width in pixels is perp_extent / √major_px2);
//          c / d are the lexicographically smallest (y, x) lesion pixels at the minimum / maximum.
// A one-pixel lesion has a = b = c = d and zeros; an empty mask has zero counts and −1 coordinates.
// lesion_px = 0xFFFFFFFF marks a slice that was not measured (it did not fit the labelling scratch).
// The derived doubles (mm, mm², degrees) exist only in measure::to_json.
struct alignas(64) SliceDiameters {
  uint32_t lesion_px;       // area of the lesion
  int32_t lesion_first[2];  // x, y of the lesion's first pixel in raster order
  uint32_t major_px2;       // squared major diameter
  uint32_t perp_extent;     // extent of the projection on n
  int32_t major[4];         // xa, ya, xb, yb
  int32_t perp[4];          // xc, yc, xd, yd
};
static_assert(sizeof(SliceDiameters) == 64, "SliceDiameters layout");
constexpr uint32_t kDiametersNotMeasured = 0xFFFFFFFFu;

// First-order intensity statistics (--measure-intensity): the record the K11 kernels write for one
// slice or one volume. The samples are the stored sample values (stored_sample below) under the DILATED
// mask, the set over which raw_sum / raw_min / raw_max are taken, so count = area_px (2D) or volume_vox
// (3D). pct[j] for p = 10, 25, 50, 75, 90 is the k-th smallest sample with k = (p · count + 99) / 100 in
// 64-bit integers (nearest rank, 1-based; p50 is the lower median of an even count). Every integer is 0
// for an empty mask. The derived doubles exist only in measure::to_json / volume_to_json.
struct alignas(64) IntensityStats {
  uint64_t count;   // samples under the mask
  uint64_t sum_sq;  // Σ v² (v² < 2^32 and count < 2^32: no overflow)
  int32_t pct[5];   // raw_p10, raw_p25, raw_p50, raw_p75, raw_p90
  uint32_t pad[7];
};
static_assert(sizeof(IntensityStats) == 64, "IntensityStats layout");

// Second-order texture (--measure-texture): the header of the record the K12 kernels write for one slice
// or one volume; the grey-level co-occurrence matrix C follows it as uint32[levels · levels], row-major
// (glcm_record_bytes). The definition is in nm03/texture_core.h: the samples are the stored sample
// values under the DILATED mask, discretised to `levels` grey levels between the smallest and the largest
// of them; C is merged over the forward directions (4 in 2D, 13 in 3D) and symmetric, Σ C = 2 · pairs.
// A record may lie at any 4-byte aligned address (odd `levels`): it is written and read as 32-bit words,
// the 64-bit fields low word first. The cells are exact while 2 · directions · samples ≤ 2^32 − 1: always
// in 2D, and for samples ≤ 165 191 049 in 3D (tcore::cells_exact). `samples` and `pairs` are 64-bit and
// stay right beyond that; a 3D record beyond it is refused by every host that reads one
// (measure::check_glcm_exact), since a cell of it may have wrapped.
struct TextureGlcm {
  uint32_t levels;   // Ng
  uint32_t key_lo;   // icore::sample_key of the smallest sample (0 for an empty mask)
  uint32_t key_hi;   // … of the largest
  uint32_t reserved;
  uint64_t samples;  // voxels under the mask
  uint64_t pairs;    // voxel pairs counted
  uint32_t pad[8];
};
static_assert(sizeof(TextureGlcm) == 64, "TextureGlcm layout");
constexpr size_t glcm_record_bytes(int levels) { return sizeof(TextureGlcm) + 4u * (size_t)levels * (size_t)levels; }

// ---------------------------------------------------------------------------------------------
// Bit quads (Gray 1971). Over every 2×2 window of the zero-padded mask, Q1 / Q3 count the windows
// with exactly one / three set pixels and QD the two diagonal patterns. The Euler number
// (components − holes, holes at the dual connectivity) is (Q1 − Q3 − 2·QD) / 4 at 8-connectivity and
// (Q1 − Q3 + 2·QD) / 4 at 4-connectivity. A w × h mask has (w + 1) × (h + 1) windows; on bit planes
// (LSB = left-most pixel) the window whose right column is pixel x sits at bit x.
// ---------------------------------------------------------------------------------------------
struct QuadCounts {
  uint32_t q1 = 0, q3 = 0, qd = 0;
};

// 64 windows at once: bit x of tl / tr / bl / br is the window's top-left / top-right / bottom-left /
// bottom-right pixel.
NM03_HD void quad_accumulate(uint64_t tl, uint64_t tr, uint64_t bl, uint64_t br, QuadCounts& q) {
  const uint64_t odd = tl ^ tr ^ bl ^ br;                 // one or three set
  const uint64_t three = odd & ((tl & tr) | (bl & br));   // three set ⇔ odd and one row of the window full
  q.q1 += (uint32_t)__builtin_popcountll(odd & ~three);
  q.q3 += (uint32_t)__builtin_popcountll(three);
  q.qd += (uint32_t)__builtin_popcountll((tl & br & ~tr & ~bl) | (tr & bl & ~tl & ~br));
}

// The windows of word k of one row pair: `u` / `l` are word k of the upper / lower row (0 for the
// padding rows above and below the mask, and masked to the width in the last word), `u_prev` /
// `l_prev` word k − 1 (0 for k = 0). `closes_row`: k is the last word and the width is a multiple of
// 64, so the window right of the last pixel (bit 0 of a word that does not exist) is counted here.
NM03_HD void quad_word(uint64_t u_prev, uint64_t u, uint64_t l_prev, uint64_t l, bool closes_row, QuadCounts& q) {
  quad_accumulate((u << 1) | (u_prev >> 63), u, (l << 1) | (l_prev >> 63), l, q);
  if (closes_row) quad_accumulate(u >> 63, 0ull, l >> 63, 0ull, q);
}

NM03_HD int64_t euler_from_quads(const QuadCounts& q, int connectivity) {
  const int64_t d = 2 * (int64_t)q.qd;
  return ((int64_t)q.q1 - (int64_t)q.q3 + (connectivity == 8 ? -d : d)) / 4;
}

// Mask of the valid bits of word k of a row of width w.
NM03_HD uint64_t row_word_mask(int k, int w) {
  const int rem = w - (k << 6);
  return rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
}

// Stored sample value as golden::SliceInput holds it: unsigned data masked to stored_bits, signed
// data sign-extended from stored_bits.
NM03_HD int32_t stored_sample(uint16_t raw_bits, uint8_t type, uint8_t stored_bits) {
  const int sh = 16 - (int)stored_bits;
  if (type == kI16) return (int32_t)(int16_t)((int16_t)(uint16_t)(raw_bits << sh) >> sh);
  return (int32_t)(raw_bits & (uint16_t)(0xFFFFu >> sh));
}

// ---------------------------------------------------------------------------------------------
// 3D volumetry (--measure-volume): the record the K8 kernels write for one volume. Exact integers,
// measured on the DILATED volume (the mask the `_processed.jpg` planes show) plus the popcount of the
// region volume; the derived doubles (mm³, mm², centroid, mean) exist only in measure::volume_to_json.
// ---------------------------------------------------------------------------------------------
struct alignas(64) VolumeMeasure {
  uint64_t volume_vox;       // popcount(dilated)
  uint64_t region_vox;       // popcount(region)
  int32_t bbox[6];           // x0, y0, z0, x1, y1, z1 inclusive; all −1 for an empty mask
  uint32_t components;       // connected components at the measurement connectivity (6 | 26)
  uint32_t cavities;         // background components that reach no frame face, at the dual connectivity
  uint64_t sum_x, sum_y, sum_z;        // coordinate sums over mask voxels
  uint64_t faces_x, faces_y, faces_z;  // voxel faces normal to each axis between mask and non-mask / frame
  uint64_t largest_vox;      // voxels of the largest component
  int64_t euler;             // Euler number at the measurement connectivity (components − tunnels + cavities)
  int64_t raw_sum;           // over the stored sample values under the mask (0 / 0 / 0 when empty)
  int32_t raw_min, raw_max;
};
static_assert(sizeof(VolumeMeasure) == 128, "VolumeMeasure layout");

// One lesion of the dilated volume (--measure-volume-lesions N): the record the K10 kernels write for
// each of the N largest connected components at the measurement connectivity. Order: voxels
// descending; a tie goes to the lesion whose first voxel in raster (z, y, x) order comes first. Exact
// integers with the definitions of the global record, so over ALL components they add up to it: a face
// between a mask voxel and a non-mask voxel (or the frame) belongs to the mask voxel's lesion.
struct alignas(64) VolumeLesion {
  uint64_t voxels;                     // voxel count
  int32_t first[3];                    // x, y, z of the first voxel in raster order
  int32_t bbox[6];                     // x0, y0, z0, x1, y1, z1 inclusive
  uint64_t sum_x, sum_y, sum_z;        // coordinate sums
  uint64_t faces_x, faces_y, faces_z;  // voxel faces normal to each axis against non-mask / the frame
  int64_t raw_sum;                     // over the stored sample values under the lesion
  int32_t raw_min, raw_max;
};
static_assert(sizeof(VolumeLesion) == 128, "VolumeLesion layout");
constexpr int kMaxVolumeLesions = 64;

// The lengths of one lesion (K13, k13_volume_diameters.hip): one record per VolumeLesion record, in the
// same order. Exact integers. The spacing enters as integer micrometres u = max(1, llround(mm · 1000))
// per axis (volume_spacing_um); every (dim − 1) · u stays below 2^31, so a squared distance is a sum of
// three squares below 2^62 and exact in 64 bits.
//   major              the pair (a, b) of lesion voxels, centre to centre, that maximises
//                      major_um2 = (dx·ux)² + (dy·uy)² + (dz·uz)²; a does not follow b in raster
//                      (z, y, x) order; a tie goes to the smallest (za, ya, xa, zb, yb, xb)
//   axial              over every plane z and every pair of the lesion's voxels of that plane (connected
//                      in the plane or not), the pair that maximises axial_um2 = (dx·ux)² + (dy·uy)²; a tie
//                      goes to the smallest z, then the smallest (ya, xa, yb, xb)
//   axial_perp         with (dx, dy) = b − a of the axial pair in index units, every lesion voxel of plane
//                      axial_z projects to p = −dy·x + dx·y; axial_perp_extent = max p − min p, and c / d
//                      are the smallest (y, x) voxels at the minimum / maximum. (The physical normal is
//                      (−dy·uy, dx·ux), whose product with (x·ux, y·uy) is ux·uy·p.)
// A one-voxel lesion has a = b = c = d and zeros; a lesion with one voxel per plane has axial_um2 = 0
// in its first plane. Worked example: the box x 0…9, y 0…3, z 0…2 at 1 mm gives major_um2 = 94 000 000,
// major = [0,0,0, 9,3,2] (four body diagonals tie), axial_z = 0, axial_um2 = 90 000 000,
// axial = [0,0, 9,3], axial_perp_extent = 54, axial_perp = [9,0, 0,3].
struct alignas(64) VolumeLesionDiameters {
  uint64_t major_um2, axial_um2;
  int64_t axial_perp_extent;
  int32_t major[6];       // xa, ya, za, xb, yb, zb
  int32_t axial_z;
  int32_t axial[4];       // xa, ya, xb, yb
  int32_t axial_perp[4];  // xc, yc, xd, yd
  int32_t pad[11];
};
static_assert(sizeof(VolumeLesionDiameters) == 128, "VolumeLesionDiameters layout");

// Euler number of a bit volume from window counts over the zero-padded volume: n3 = set voxels,
// n2 = pairs of face-adjacent positions, n1 = 2×2 windows (three orientations), n0 = 2×2×2 windows.
// At 26-connectivity a pair or window counts when ANY of its voxels is set and
// euler = n0 − n1 + n2 − n3; at 6-connectivity when ALL are set and euler = n3 − n2 + n1 − n0.
// The window whose highest corner is voxel (x, y, z) sits at bit x of word (y, z), as in 2D.
struct EulerCounts {
  uint64_t n2 = 0, n1 = 0, n0 = 0;
};

// 64 window positions at once. a[0..3]: the word of row (y, z), (y − 1, z), (y, z − 1), (y − 1, z − 1);
// s[0..3]: the same rows one voxel to the left (bit x = voxel x − 1).
NM03_HD void euler_accumulate(bool all, const uint64_t a[4], const uint64_t s[4], EulerCounts& e) {
  uint64_t px, py, pz, wxy, wxz, wyz, cube;
  if (all) {
    px = a[0] & s[0], py = a[0] & a[1], pz = a[0] & a[2];
    wxy = px & a[1] & s[1], wxz = px & a[2] & s[2], wyz = py & a[2] & a[3];
    cube = wxy & a[2] & s[2] & a[3] & s[3];
  } else {
    px = a[0] | s[0], py = a[0] | a[1], pz = a[0] | a[2];
    wxy = px | a[1] | s[1], wxz = px | a[2] | s[2], wyz = py | a[2] | a[3];
    cube = wxy | a[2] | s[2] | a[3] | s[3];
  }
  e.n2 += (uint64_t)(__builtin_popcountll(px) + __builtin_popcountll(py) + __builtin_popcountll(pz));
  e.n1 += (uint64_t)(__builtin_popcountll(wxy) + __builtin_popcountll(wxz) + __builtin_popcountll(wyz));
  e.n0 += (uint64_t)__builtin_popcountll(cube);
}

// The windows of word k at position (y, z): `cur` / `prev` hold word k / k − 1 (0 for k = 0) of the
// four rows in euler_accumulate's order, masked to the width and 0 outside the volume — so y = h and
// z = d (the padding row and plane past the last voxel) are positions like any other. `closes_row`:
// k is the last word and the width is a multiple of 64, so the windows right of the last voxel (bit 0
// of a word that does not exist) are counted here.
NM03_HD void euler_word(bool all, const uint64_t cur[4], const uint64_t prev[4], bool closes_row, EulerCounts& e) {
  uint64_t s[4];
  for (int r = 0; r < 4; ++r) s[r] = (cur[r] << 1) | (prev[r] >> 63);
  euler_accumulate(all, cur, s, e);
  if (closes_row) {
    const uint64_t zero[4] = {0ull, 0ull, 0ull, 0ull};
    for (int r = 0; r < 4; ++r) s[r] = cur[r] >> 63;
    euler_accumulate(all, zero, s, e);
  }
}

NM03_HD int64_t euler_from_counts(const EulerCounts& e, uint64_t n3, int connectivity) {
  const int64_t v = (int64_t)n3 - (int64_t)e.n2 + (int64_t)e.n1 - (int64_t)e.n0;
  return connectivity == 6 ? v : -v;
}

// Words of K8's labelling scratch: one slot per voxel plus one per row (rows are w + 1 slots apart),
// one more for the last area slot. 0 when the slots cannot be named by 32-bit indices.
inline size_t volume_measure_scratch_words(int w, int h, int d) {
  if (w <= 0 || h <= 0 || d <= 0) return 0;
  const uint64_t row_slots = ((uint64_t)w + 1) * (uint64_t)h;  // < 2^63
  if (row_slots > (0xFFFFFFFFull - 1) / (uint64_t)d) return 0;  // (w + 1)·h·d + 1 ≥ 2^32
  return (size_t)(row_slots * (uint64_t)d + 1);
}

namespace measure {

// The sidecar text of a volume record (volume_measure.json): one JSON object on one line plus '\n',
// keys in fixed order — width, height, depth, connectivity, the record's integers (bbox as
// [x0, y0, z0, x1, y1, z1]), tunnels = components + cavities − euler, then spacing_x / _y / _z,
// spacing_z_source and the derived doubles, each printed with %.9g:
//   volume_mm3 = volume_vox · sx · sy · sz, volume_ml = volume_mm3 / 1000
//   surface_mm2 = faces_x · sy · sz + faces_y · sx · sz + faces_z · sx · sy
//   centroid_x / _y / _z = sum / volume_vox (voxel indices), centroid_*_mm = centroid · spacing
//   mean = raw_sum / volume_vox, mapped through slope · v + intercept when apply_rescale
// Centroids and mean are null for an empty mask. The GPU path, the --cpu path and the Python
// bindings all call this one function.
std::string volume_to_json(const VolumeMeasure& m, int w, int h, int d, double spacing_x, double spacing_y,
                           double spacing_z, const std::string& spacing_z_source, float slope, float intercept,
                           bool apply_rescale, int connectivity);

// The record of a bit volume (d planes of h rows of wpr words) computed on the host with the word
// arithmetic and the run union-find that the K8 kernels use (nm03/volume_measure_core.h), one word
// after the other: what the kernels compute, without a GPU.
VolumeMeasure volume_words(const uint64_t* dilated, const uint64_t* region, const uint16_t* raw, size_t raw_plane_stride,
                           int w, int h, int d, int wpr, uint8_t type, uint8_t stored_bits, int connectivity);

// The sidecar text with --measure-volume-lesions: the text above with two keys after `mean` —
// lesions_max (the N asked for) and lesions, an array of `count` objects in the records' order, each
// with keys in fixed order: voxels, first [x, y, z], bbox [x0, y0, z0, x1, y1, z1], sum_x / _y / _z,
// faces_x / _y / _z, raw_sum, raw_min, raw_max, then the derived doubles (%.9g): volume_mm3,
// volume_ml, surface_mm2 (the formulas above on the lesion's integers), equivalent_diameter_mm =
// cbrt(6 · volume_mm3 / π), centroid_x / _y / _z, centroid_*_mm and mean.
std::string volume_to_json(const VolumeMeasure& m, const VolumeLesion* lesions, int count, int lesions_max, int w, int h,
                           int d, double spacing_x, double spacing_y, double spacing_z,
                           const std::string& spacing_z_source, float slope, float intercept, bool apply_rescale,
                           int connectivity);

// The `max_lesions` largest components of a bit volume computed on the host with the per-word lesion
// logic of the K10 kernels (nm03/volume_measure_core.h: root keys, stretch figures) on K8's run
// union-find, one word after the other. Returns the reported count, min(max_lesions, components).
int volume_lesions_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                         int wpr, uint8_t type, uint8_t stored_bits, int connectivity, int max_lesions, VolumeLesion* out);

// The spacing of a volume in integer micrometres, max(1, llround(mm · 1000)) per axis (x, y, z).
void volume_spacing_um(double spacing_x, double spacing_y, double spacing_z, uint32_t um[3]);
// Empty when every (dim − 1) · u stays below 2^31, else the message that names the offending product.
std::string volume_diameters_extent_error(int w, int h, int d, const uint32_t um[3]);

// The VolumeLesionDiameters records of the `max_lesions` largest components of a bit volume computed on
// the host with the K13 kernels' logic (nm03/volume_diameters_core.h: the row extremes of every in-word
// stretch, the direction bound, the tile boxes and the tile rule) on K8's run union-find and K10's
// selection, one word / tile pair after the other. `brute_force` compares every tile pair. Returns the
// reported count; `skipped` (optional) receives the number of tile pairs the bound skipped.
int volume_diameters_words(const uint64_t* dilated, int w, int h, int d, int wpr, int connectivity, int max_lesions,
                           const uint32_t um[3], bool brute_force, VolumeLesionDiameters* out,
                           uint64_t* skipped = nullptr);

// The sidecar text with --measure-volume-diameters: `text` (any volume_to_json text with the lesion keys)
// with one top-level key directly before lesions_max — diameters_spacing_um [ux, uy, uz] — and inside
// lesion object i, after `mean`, the integers of dia[i] in fixed order — major_um2, major
// [xa, ya, za, xb, yb, zb], axial_z, axial_um2, axial [xa, ya, xb, yb], axial_perp_extent, axial_perp
// [xc, yc, xd, yd] — then the derived doubles (%.9g), from the integers and the quantised spacing alone:
//   diameter_3d_mm = √major_um2 / 1000, axial_major_mm = √axial_um2 / 1000,
//   axial_perp_mm = ux · uy · axial_perp_extent / √axial_um2 / 1000 (0 when axial_um2 is 0),
//   axial_bidimensional_mm2 = axial_major_mm · axial_perp_mm
// Removing the new keys gives `text` back byte for byte. `count` must be the text's lesion count.
std::string insert_diameter_keys(std::string text, const VolumeLesionDiameters* dia, int count, const uint32_t um[3]);
// The four doubles of a record.
struct DiameterLengths {
  double diameter_3d_mm, axial_major_mm, axial_perp_mm, axial_bidimensional_mm2;
};
DiameterLengths diameter_lengths(const VolumeLesionDiameters& r, const uint32_t um[3]);

inline const char* volume_sidecar_name() { return "volume_measure.json"; }

// Euler number of a bit plane (h rows of wpr words, bits past w ignored) from the quad counts above.
int64_t euler_plane(const uint64_t* plane, int w, int h, int wpr, int connectivity);

// The sidecar text: one JSON object on one line plus '\n', keys in fixed order — the slice's width,
// height and the connectivity, the record's integers (bbox as [x0, y0, x1, y1]), then the derived
// doubles, each printed with %.9g:
//   area_mm2 = area_px · spacing_x · spacing_y
//   centroid_x / centroid_y = sum / area_px (pixel indices), centroid_*_mm = centroid · spacing
//   mean = raw_sum / area_px, mapped through slope · v + intercept when apply_rescale
// Centroids and mean are null for an empty mask.
std::string to_json(const SliceMeasure& m, int w, int h, float spacing_x, float spacing_y, float slope, float intercept,
                    bool apply_rescale, int connectivity);

// The sidecar text with --measure-diameters: the text above with the diameter record's keys after
// `mean` — lesion_px, lesion_first [x, y], major_px2, major [xa, ya, xb, yb], perp_extent,
// perp [xc, yc, xd, yd], then the derived doubles (%.9g), with u = ((xb − xa)·sx, (yb − ya)·sy) and
// v = ((xd − xc)·sx, (yd − yc)·sy):
//   major_mm = |u|, perp_mm = |u × v| / |u| (0 when |u| = 0), bidimensional_mm2 = major_mm · perp_mm,
//   major_angle_deg = atan2(u.y, u.x) in degrees (null when |u| = 0)
// All four are null for an empty mask. The pair (a, b) is maximal in PIXEL space: it is the mm-space
// maximum when the spacing is isotropic.
std::string to_json(const SliceMeasure& m, const SliceDiameters& d, int w, int h, float spacing_x, float spacing_y,
                    float slope, float intercept, bool apply_rescale, int connectivity);

// The sidecar texts with --measure-intensity: the texts above with the intensity keys appended — after
// `mean` (after the diameter keys when there are any; in 3D before lesions_max / lesions), so the text
// before the new keys is byte for byte the text without them. First the integers: raw_sum_sq, raw_p10,
// raw_p25, raw_p50, raw_p75, raw_p90; then the derived doubles (%.9g):
//   std = √((n · sum_sq − raw_sum²) / n²), the population standard deviation, the numerator formed
//         exactly in 128-bit integers; times |slope| when apply_rescale
//   p10, p25, median, p75, p90 = slope · raw_pP + intercept when apply_rescale, else raw_pP
//   iqr = |p75 − p25|
// With a negative slope these are the MAPPED raw order statistics (p10 > p90), as `mean` is the mapped
// raw mean. All seven are null for an empty mask.
std::string to_json(const SliceMeasure& m, const IntensityStats& st, int w, int h, float spacing_x, float spacing_y,
                    float slope, float intercept, bool apply_rescale, int connectivity);
std::string to_json(const SliceMeasure& m, const SliceDiameters& d, const IntensityStats& st, int w, int h, float spacing_x,
                    float spacing_y, float slope, float intercept, bool apply_rescale, int connectivity);
std::string volume_to_json(const VolumeMeasure& m, const IntensityStats& st, int w, int h, int d, double spacing_x,
                           double spacing_y, double spacing_z, const std::string& spacing_z_source, float slope,
                           float intercept, bool apply_rescale, int connectivity);
std::string volume_to_json(const VolumeMeasure& m, const IntensityStats& st, const VolumeLesion* lesions, int count,
                           int lesions_max, int w, int h, int d, double spacing_x, double spacing_y, double spacing_z,
                           const std::string& spacing_z_source, float slope, float intercept, bool apply_rescale,
                           int connectivity);
// The population standard deviation of the raw samples, √(n · sum_sq − raw_sum²) / n with the radicand
// exact in 128-bit integers; 0 for an empty mask.
double intensity_std(const IntensityStats& st, int64_t raw_sum);
// The appended keys alone (",\"raw_sum_sq\":…" up to iqr), for the overloads above.
std::string intensity_keys(const IntensityStats& st, int64_t raw_sum, float slope, float intercept, bool apply_rescale);

// The record of the samples under a bit plane (h rows of wpr words) or, with d > 1 planes of h · wpr
// words and the samples of plane z at raw + z · raw_plane_stride, a bit volume, computed on the host
// with the two-pass radix select of nm03/intensity_core.h, one word after the other: what the K11
// kernels compute, without a GPU.
IntensityStats intensity_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d,
                               int wpr, uint8_t type, uint8_t stored_bits);

// ---- texture (--measure-texture, nm03/texture_core.h) ------------------------------------------------
// A record on the host: the header and the matrix.
struct Glcm {
  TextureGlcm head = {};
  std::vector<uint32_t> c;  // levels · levels, row-major
};
// A record as the kernels write it (header, then the matrix) read from 32-bit words at `p`.
Glcm glcm_from_record(const void* p);
// Throws std::invalid_argument when a 3D record of `samples` voxels may hold a wrapped 32-bit cell
// (tcore::cells_exact over the thirteen directions): one message, naming the bound, for the volume
// runner, the ops binding, the golden model and texture_words.
void check_glcm_exact(uint64_t samples);

// Everything the sidecar derives from a matrix, by ONE function in a fixed loop order (i, then j,
// row-major), so equal matrices give equal text whoever computed them. With p = C / Σ C and IBSI's
// 1-based grey levels i, j. The integers first; `any` is false when pairs = 0 and every double is then
// null in the text; `correlation_defined` is false when joint_var = 0.
struct GlcmFeatures {
  uint64_t levels = 0, pairs = 0, nonzero = 0, max_count = 0, sum_abs_d = 0, sum_d2 = 0, sum_sq = 0;
  bool any = false, correlation_defined = false;
  double joint_max = 0, joint_avg = 0, joint_var = 0, joint_entropy = 0, asm_ = 0, contrast = 0, dissimilarity = 0,
         inv_diff = 0, inv_diff_moment = 0, correlation = 0, autocorrelation = 0, cluster_tendency = 0, cluster_shade = 0,
         cluster_prominence = 0, sum_entropy = 0, diff_entropy = 0;
};
GlcmFeatures glcm_features(const uint32_t* c, int levels);
// The appended keys alone: ",\"glcm_levels\":…" up to glcm_diff_entropy (7 integers, then 16 doubles as %.9g or null).
std::string texture_keys(const uint32_t* c, int levels);
// The sidecar texts with --measure-texture: the text of the matching overload without `tx` (d, st, lesions:
// null for a run without that flag) with the texture keys after all existing keys — in 3D before
// lesions_max / lesions — so the text before them is byte for byte the text without the flag.
std::string to_json(const SliceMeasure& m, const SliceDiameters* d, const IntensityStats* st, const Glcm& tx, int w, int h,
                    float spacing_x, float spacing_y, float slope, float intercept, bool apply_rescale, int connectivity);
std::string volume_to_json(const VolumeMeasure& m, const IntensityStats* st, const VolumeLesion* lesions, int count,
                           int lesions_max, const Glcm& tx, int w, int h, int d, double spacing_x, double spacing_y,
                           double spacing_z, const std::string& spacing_z_source, float slope, float intercept,
                           bool apply_rescale, int connectivity);
// `text` (a slice's or a volume's sidecar) with `keys` put after its global keys: before the lesion keys
// when it has them, else before the closing brace.
std::string insert_global_keys(std::string text, const std::string& keys);

// The record of the samples under a bit plane or (d > 1) a bit volume, laid out as for intensity_words,
// computed on the host with K12's per-word pair logic (tcore::neighbour_word over the five partner
// rows, directed counts, one symmetrisation): what the K12 kernels compute, without a GPU.
Glcm texture_words(const uint64_t* dilated, const uint16_t* raw, size_t raw_plane_stride, int w, int h, int d, int wpr,
                   uint8_t type, uint8_t stored_bits, int levels);

// File name of a slice's sidecar next to its JPEGs.
inline std::string sidecar_name(const std::string& stem) { return stem + "_measure.json"; }

}  // namespace measure
}  // namespace nm03
