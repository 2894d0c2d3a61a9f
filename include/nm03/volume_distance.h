// nm03/volume_distance.h — the exact Euclidean distance map of a 3D mask in physical space (K16), with its
// two first consumers: a margin in millimetres (--dilate-mm) and the thickness of the dilated volume
// (--measure-volume-thickness).
//
// DEFINITIONS (the README and the tests quote these)
//   Spacing.           U = (ux, uy, uz) = measure::volume_spacing_um(sx, sy, sz), integer micrometres (K13's rule).
//   Squared distance.  d²(p, q) = ((px − qx)·ux)² + ((py − qy)·uy)² + ((pz − qz)·uz)², voxel centre to voxel
//                      centre, in 64-bit integers.
//   Extent rule.       A volume with ((w − 1)·ux)² + ((h − 1)·uy)² + ((d − 1)·uz)² ≥ 2^62 is refused on the host
//                      before any launch, with a message that names the sum. Below that bound every intermediate,
//                      differences of two distances included, fits a signed 64-bit integer.
//   Distance map       of a set S of voxels of the frame: D_S(p) = min over q ∈ S of d²(p, q). It is 0 exactly on
//                      S. kNoDistance = 2^63 − 1 stands at every p when S is empty. With a cap c (µm, ≥ 0) every
//                      value above c² is replaced by kNoDistance. S is either the set voxels of a mask
//                      ("foreground") or its zero voxels inside the frame ("background"). OUTSIDE THE FRAME IS
//                      NEITHER (SciPy's distance_transform_edt convention).
//   Margin.            r = llround(R · 1000) µm, dilated = { p : D_region(p) ≤ r² }. R = 0 gives the region
//                      itself. One voxel at (10, 10, 2) of a 21 × 21 × 5 volume at 0.5 × 0.5 × 5 mm, R = 5, gives
//                      319 voxels: 317 in its plane (dx² + dy² ≤ 100) plus the one directly above and below. At
//                      1 mm isotropic R = 3 gives the 123-voxel digital ball; for isotropic spacing s and R = k·s
//                      the margin equals golden::dilate3d(region, …, 2k + 1, ball = true).
//   Thickness          of a mask M: inscribed_um2 = max over p ∈ M of D_background(p); inscribed_at is the p that
//                      attains it, a tie goes to the smallest raster (z, y, x); inscribed_radius_mm =
//                      √inscribed_um2 / 1000; thickness_mm = 2 · inscribed_radius_mm. Distances are centre to
//                      centre, so a slab n voxels thick along x reports (⌊(n − 1) / 2⌋ + 1)·ux as its radius. An
//                      empty mask, or a mask with no background voxel in the frame, has 0 for the integer, −1
//                      coordinates and null derived values.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/measure.h"

namespace nm03 {

constexpr int64_t kNoDistance = INT64_MAX;  // 2^63 − 1
constexpr double kMaxDilateMm = 1000.0;     // --dilate-mm R: 0 ≤ R ≤ 1000
constexpr int64_t kMaxDilateUm = 1000000;

// The thickness record, as K16's last launch writes it (plain vector stores; device, pinned or host-mapped).
struct alignas(32) VolumeThickness {
  uint64_t inscribed_um2;  // 0 when !found
  int32_t at[3];           // x, y, z; −1 when !found
  int32_t found;           // 1 when the mask has a voxel and the frame a background voxel
  uint64_t pad;
};
static_assert(sizeof(VolumeThickness) == 32, "VolumeThickness layout");

namespace measure {

// Empty when ((w − 1)·ux)² + ((h − 1)·uy)² + ((d − 1)·uz)² stays below 2^62, else the message that names the sum.
std::string volume_distance_extent_error(int w, int h, int d, const uint32_t um[3]);

// r = llround(R · 1000): the margin in micrometres.
int64_t dilate_mm_to_um(double mm);

// The distance map of a bit volume (d planes of h rows of wpr words, bits past w ignored) computed on the
// host with the per-line functions of the K16 kernels (nm03/volume_distance_core.h: the in-word nearest
// bit, the word walk, the outward search with its stop rule), one voxel after the other: what the kernels
// compute, without a GPU. cap_um < 0 = no cap. `out`: w · h · d values, raster (z, y, x).
void volume_distance_words(const uint64_t* bits, int w, int h, int d, int wpr, const uint32_t um[3], bool to_background,
                           int64_t cap_um, int64_t* out);
// The thickness of the same bit volume from that map, with the kernels' (value, position) order.
VolumeThickness volume_thickness_words(const uint64_t* bits, int w, int h, int d, int wpr, const uint32_t um[3]);

// The appended keys alone: ",\"thickness_spacing_um\":[ux,uy,uz],\"inscribed_um2\":…,\"inscribed_at\":[x,y,z],
// \"inscribed_radius_mm\":…,\"thickness_mm\":…" (%.9g, or null when nothing was found).
std::string thickness_keys(const VolumeThickness& t, const uint32_t um[3]);
// The sidecar text with --measure-volume-thickness: `text` (any volume_to_json text) with the thickness keys
// after the texture keys (after the intensity keys, or `mean`, when those are absent) and before
// diameters_spacing_um / lesions_max. Removing them gives `text` back byte for byte.
std::string insert_thickness_keys(std::string text, const VolumeThickness& t, const uint32_t um[3]);
// √inscribed_um2 / 1000 (0 when nothing was found).
double inscribed_radius_mm(const VolumeThickness& t);

}  // namespace measure

namespace golden {

// The distance map by three plain passes that minimise over the WHOLE line, with no stop rule: independent
// of the kernels' pruning. `mask`: w · h · d bytes, non-zero = set. cap_um < 0 = no cap.
std::vector<int64_t> volume_distance(const std::vector<uint8_t>& mask, int w, int h, int d, const uint32_t um[3],
                                     bool to_background, int64_t cap_um);
// The margin by the direct definition: every region voxel with an open 6-face ORs the precomputed list of
// offsets with d² ≤ r² (the others are copied). Not a threshold of the map.
std::vector<uint8_t> dilate3d_mm(const std::vector<uint8_t>& region, int w, int h, int d, const uint32_t um[3], int64_t r_um);
// Plain loops over volume_distance(mask, …, to_background = true, no cap).
VolumeThickness volume_thickness(const std::vector<uint8_t>& mask, int w, int h, int d, const uint32_t um[3]);

}  // namespace golden
}  // namespace nm03
