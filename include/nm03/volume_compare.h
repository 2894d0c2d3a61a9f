// nm03/volume_compare.h — overlap and surface distances between two 3D masks of one frame (K17, --compare-to).
//
// DEFINITIONS (the README and the tests quote these)
//   A is the run's dilated mask, B the reference mask of the same w × h × d. U = (ux, uy, uz) =
//   measure::volume_spacing_um of the series' spacing; d² is the squared distance of nm03/volume_distance.h.
//   Overlap.           a_vox = |A|, b_vox = |B|, tp_vox = |A ∩ B|, fp_vox = |A \ B|, fn_vox = |B \ A|.
//   Surface.           S(M) = the voxels of M with at least one of their six face neighbours not in M; a
//                      neighbour outside the frame counts as not in M (K10's convention for open faces). It equals
//                      M ^ binary_erosion(M, generate_binary_structure(3, 1)) of SciPy. A mask that fills a
//                      3 × 3 × 3 frame has 26 surface voxels, a 5³ cube inside a 7³ frame 98.
//   Surface distance.  Surface to surface (MedPy's convention), not surface to voxel: for p ∈ S(A),
//                      D(p) = min over q ∈ S(B) of d²(p, q), K16's foreground map of the bit volume S(B) with no
//                      cap. A surface voxel of A deep inside B has a positive distance.
//   Integer distance.  s(p) = ⌊√D(p)⌋ in whole micrometres, an exact integer square root
//                      (vcmp::isqrt_um of nm03/volume_compare_core.h). K16's extent rule keeps D below 2^62, so
//                      s < 2^31 fits a 32-bit key.
//   Directed record    A→B: n = |S(A)|; max_um2 = max D; worst = the p that attains it, a tie goes to the smallest
//                      raster (z, y, x); sum_um = Σ s(p); p95_um = the k-th smallest s with k = (95·n + 99) / 100
//                      (K11's nearest rank, icore::percentile_rank); found = 1 when BOTH surfaces are non-empty,
//                      otherwise every integer is 0 and worst is −1. B→A alike with the roles swapped.
//   Derived values     (%.9g; null when the denominator is 0 or a direction was not found):
//                      dice = 2·tp / (a + b), jaccard = tp / (a + b − tp), sensitivity = tp / b, precision = tp / a;
//                      volume_a_mm3, volume_b_mm3, volume_diff_mm3 (a − b);
//                      hausdorff_mm = √max(max_um2_ab, max_um2_ba) / 1000;
//                      hd95_mm = max(p95_um_ab, p95_um_ba) / 1000, the larger of the two directed percentiles (the
//                      BraTS convention), not a percentile of the pooled set;
//                      msd_ab_mm = sum_um_ab / n_ab / 1000, msd_ba_mm alike;
//                      assd_mm = (sum_um_ab + sum_um_ba) / (n_ab + n_ba) / 1000.
//                      s is floored to whole micrometres, so the mean distances lie below the real-valued ones by
//                      less than 0.001 mm.
//
// WORKED EXAMPLES (computed with SciPy; tests/volume_compare_cases.py holds them)
//   1. 16 × 8 × 5 at U = (1000, 1000, 2500). A = box x 0…9, y 0…3, z 0…2; B = box x 2…13, y 1…6, z 1…4 plus the
//      voxel (15, 6, 4). a 120, b 289, tp 48, fp 72, fn 241; |S(A)| = 104, |S(B)| = 209.
//      A→B: max_um2 11 250 000 (⌊√⌋ 3354), sum_um 164 741, p95_um 2692 (k = 99).
//      B→A: max_um2 70 000 000 (⌊√⌋ 8366), sum_um 716 543, p95_um 5916 (k = 199).
//   2. Nested boxes at 1 mm in an 11³ frame: A = 3³ at 4…6, B = 9³ at 1…9. tp 27. A→B: n 26, every s = 3000, so
//      sum_um 78 000, max_um2 9 000 000, p95_um 3000 (surface to voxel would give 0). B→A: n 386, max_um2
//      27 000 000, sum_um 1 418 760, p95_um 4690.
//   3. Keys above 2^24: 8 × 1 × 1 at U = (4 000 000, 1000, 1000), A = {x 0}, B = {x 7}. Both directions: n 1,
//      max_um2 784 000 000 000 000, s = 28 000 000.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/measure.h"
#include "nm03/volume_distance.h"

namespace nm03 {

struct VolumeCompareLesions;  // nm03/volume_compare_lesions.h (K18, --compare-lesions)

struct VolumeCompareDirected {
  uint64_t max_um2;  // 0 when !found
  uint64_t sum_um;   // Σ ⌊√D⌋
  uint32_t n;        // |S(from)| when found, else 0
  uint32_t p95_um;
  int32_t worst[3];  // x, y, z; −1 when !found
  int32_t found;     // 1 when both surfaces are non-empty
};
static_assert(sizeof(VolumeCompareDirected) == 40, "VolumeCompareDirected layout");

// The comparison record, as K17's last launches write it (plain vector stores; device, pinned or host-mapped).
struct alignas(16) VolumeCompare {
  uint64_t a_vox, b_vox, tp_vox, fp_vox, fn_vox;
  uint64_t surface_a, surface_b;
  VolumeCompareDirected ab, ba;
  uint64_t pad;
};
static_assert(sizeof(VolumeCompare) == 144, "VolumeCompare layout");

namespace measure {

// The comparison of two bit volumes (d planes of h rows of wpr words, bits past w ignored) computed on the host
// with the functions of the K17 kernels (nm03/volume_compare_core.h: the surface word, the integer square
// root, the digits of the radix select with icore::select_bin, the (value, position) order) over K16's host map
// (measure::volume_distance_words): what the kernels compute, without a GPU. When `surface_a` / `surface_b` are
// given they receive the surface words (every word written, bits past the width zero).
VolumeCompare volume_compare_words(const uint64_t* a, const uint64_t* b, int w, int h, int d, int wpr, const uint32_t um[3],
                                   uint64_t* surface_a = nullptr, uint64_t* surface_b = nullptr);

}  // namespace measure

namespace compare {

// hausdorff_mm and the like as doubles; `ok` false where the JSON says null.
struct Derived {
  double dice, jaccard, sensitivity, precision, volume_a_mm3, volume_b_mm3, volume_diff_mm3, hausdorff_mm, hd95_mm, msd_ab_mm,
      msd_ba_mm, assd_mm;
  bool dice_ok, jaccard_ok, sensitivity_ok, precision_ok, distances_ok;
};
Derived derive(const VolumeCompare& c, const uint32_t um[3]);

// The one writer of compare.json (GPU path, --cpu and Python): one object on one line, keys in fixed order —
// width, height, depth, compare_spacing_um, reference; a_vox, b_vox, tp_vox, fp_vox, fn_vox, surface_a, surface_b;
// n_ab, max_um2_ab, worst_ab [x, y, z], sum_um_ab, p95_um_ab, found_ab and the same for ba; then the derived
// values in the order of Derived. Ends with "}\n". With `lesions` (K18, --compare-lesions) the lesion keys of
// nm03/volume_compare_lesions.h (compare::lesions_json_keys) follow assd_mm; removing them gives the text without.
std::string to_json(const VolumeCompare& c, int w, int h, int d, const uint32_t um[3], const std::string& reference,
                    const VolumeCompareLesions* lesions = nullptr);
// comparisons.csv: the header line (no newline) and one patient's fields after "patient,status," (arrays
// flattened; the same values as to_json, null written as an empty field). With `lesions` the nine per-volume
// lesion columns (the six totals, then lesion_sensitivity, lesion_precision, lesion_f1) follow all the others.
std::string csv_header(bool lesions = false);
std::string csv_fields(const VolumeCompare& c, int w, int h, int d, const uint32_t um[3], const std::string& reference,
                       const VolumeCompareLesions* lesions = nullptr);

}  // namespace compare

namespace golden {

// Plain loops: the six-neighbour test per voxel, golden::volume_distance of the surface masks, a std::sort for
// the percentile. `a`, `b`: w · h · d bytes, non-zero = set.
VolumeCompare compare_volumes(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int w, int h, int d, const uint32_t um[3]);
// S(M) alone, 0 / 1 per voxel.
std::vector<uint8_t> volume_surface(const std::vector<uint8_t>& m, int w, int h, int d);

}  // namespace golden
}  // namespace nm03
