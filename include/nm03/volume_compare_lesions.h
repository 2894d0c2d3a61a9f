// nm03/volume_compare_lesions.h — lesion-wise detection scores for two 3D masks of one frame (K18, --compare-lesions).
//
// DEFINITIONS (the README and the tests quote these)
//   Masks.            A is the run's dilated mask, B the reference of the same w × h × d, as in nm03/volume_compare.h.
//   Lesions.          The connected components of a mask at connectivity c = --measure-volume-connectivity (6 or 26,
//                     default 26): the components K8 and K10 report. A component is named by the slot of its first
//                     voxel in raster (z, y, x) order, which is K8's root.
//   Reported lesions. For N = 1 … 64 (kMaxVolumeLesions) the N largest lesions of each mask, largest first; a tie goes
//                     to the earlier first voxel (K10's order, vmcore::lesion_key). A mask with fewer components
//                     reports that many.
//   Overlap of a lesion L with the other mask M. overlap_vox = |L ∩ M|. L is HIT when overlap_vox ≥ 1 and MULTI when
//                     it intersects at least two different components of M.
//   Totals per side,  over ALL components, not only the reported ones: lesions_a, hit_a, multi_a, lesions_b, hit_b,
//                     multi_b. hit_b counts the reference lesions that were detected and lesions_b − hit_b the missed
//                     ones; lesions_a − hit_a counts the spurious ones; multi_a counts run lesions that merge several
//                     reference lesions, multi_b reference lesions that the run split.
//   Table.            o[i][j] = |A_i ∩ B_j| for i, j in 0 … N, (N + 1)² u64 cells, row-major. Index N on either side
//                     collects all unreported components of that side. Only voxels of A ∩ B are counted, so
//                     Σ o = K17's tp_vox.
//   Record of a reported lesion, the same on both sides: voxels; first [x, y, z]; overlap_vox, its row (A) or column
//                     (B) sum, index N included; partners_reported, the reported lesions of the other side with o > 0;
//                     overlap_other_vox, its cell at index N; multi, 0 or 1; best, the index of the other side's
//                     reported lesion with the largest o, a tie going to the smaller index, −1 when
//                     partners_reported is 0; best_overlap_vox.
//   Derived values    (%.9g; null when a denominator is 0). Per lesion: coverage = overlap_vox / voxels and best_dice =
//                     2 · best_overlap_vox / (voxels + the partner's voxels). Per volume: lesion_sensitivity =
//                     hit_b / lesions_b, lesion_precision = hit_a / lesions_a, lesion_f1 = 2·hit_b /
//                     (2·hit_b + (lesions_a − hit_a) + (lesions_b − hit_b)).
//
// WORKED EXAMPLES (checkable by hand; tests/volume_compare_lesion_cases.py holds them)
//   1. K17's example 1: 16 × 8 × 5, A = box x 0…9, y 0…3, z 0…2; B = box x 2…13, y 1…6, z 1…4 plus the voxel
//      (15, 6, 4). lesions_a 1, hit_a 1, multi_a 0; lesions_b 2, hit_b 1, multi_b 0; sensitivity 0.5, precision 1,
//      f1 2/3. With N = 2: o[0][0] = 48, every other cell 0.
//   2. A 12 × 1 × 1 row at c = 6: A = {0…2}, {4…6}, {9}; B = {2…4}, {11}. lesions_a 3, hit_a 2, multi_a 0; lesions_b 2,
//      hit_b 1, multi_b 1; sensitivity 0.5, precision 2/3, f1 0.5. With N = 2, B's first lesion has voxels 3, first
//      [2, 0, 0], overlap_vox 2, partners_reported 2, overlap_other_vox 0, multi 1, best 0 (a tie), best_overlap_vox 1,
//      best_dice 1/3; B's second lesion has overlap 0 and best −1. With N = 1, B's first lesion has
//      partners_reported 1, overlap_other_vox 1, multi 1.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "nm03/measure.h"

namespace nm03 {

// One reported lesion, as K18's last launch writes it (plain vector stores).
struct VolumeCompareLesion {
  uint64_t voxels;
  uint64_t overlap_vox;
  uint64_t overlap_other_vox;
  uint64_t best_overlap_vox;
  int32_t first[3];  // x, y, z
  uint32_t partners_reported;
  int32_t multi;  // 0 or 1
  int32_t best;   // −1 = none
};
static_assert(sizeof(VolumeCompareLesion) == 56, "VolumeCompareLesion layout");

// The head of K18's record.
struct VolumeCompareLesionsHead {
  uint32_t connectivity, max_lesions;  // c and N
  uint32_t lesions_a, hit_a, multi_a, lesions_b, hit_b, multi_b;
  uint32_t reported_a, reported_b;  // min(N, lesions)
  uint32_t pad[6];
};
static_assert(sizeof(VolumeCompareLesionsHead) == 64, "VolumeCompareLesionsHead layout");

// K18's record in memory for N = max_lesions: the head, N records of A, N records of B (those past the reported
// count are zero), then the (N + 1)² cells of the table.
inline size_t volume_compare_lesions_record_bytes(int max_lesions) {
  return sizeof(VolumeCompareLesionsHead) + 2 * (size_t)max_lesions * sizeof(VolumeCompareLesion) +
         (size_t)(max_lesions + 1) * (size_t)(max_lesions + 1) * sizeof(uint64_t);
}
constexpr size_t kVolumeCompareLesionsMaxRecordBytes =
    sizeof(VolumeCompareLesionsHead) + 2 * (size_t)kMaxVolumeLesions * sizeof(VolumeCompareLesion) +
    (size_t)(kMaxVolumeLesions + 1) * (size_t)(kMaxVolumeLesions + 1) * sizeof(uint64_t);

// The record on the host: the reported lesions only, and the table.
struct VolumeCompareLesions {
  VolumeCompareLesionsHead head = {};
  std::vector<VolumeCompareLesion> a, b;  // head.reported_a / reported_b records
  std::vector<uint64_t> table;            // (N + 1)², row (A) major
  uint64_t cell(int i, int j) const { return table[(size_t)i * (size_t)(head.max_lesions + 1) + (size_t)j]; }
};

namespace measure {

// K18's record in memory → the host form.
VolumeCompareLesions unpack_compare_lesions(const void* record, int max_lesions);

// The lesion-wise comparison of two bit volumes (d planes of h rows of wpr words, bits past w ignored) computed on
// the host with the functions of the K18 kernels (nm03/volume_measure_core.h for the labelling,
// nm03/volume_compare_lesions_core.h for the join, the partner cells, the rank lookup and the best partner), a word
// after the other: what the kernels compute, without a GPU.
VolumeCompareLesions volume_compare_lesions_words(const uint64_t* a, const uint64_t* b, int w, int h, int d, int wpr, int max_lesions,
                                                  int connectivity);

}  // namespace measure

namespace compare {

struct LesionsDerived {
  double sensitivity, precision, f1;
  bool sensitivity_ok, precision_ok, f1_ok;
};
LesionsDerived derive_lesions(const VolumeCompareLesions& l);

// compare.json's keys after assd_mm, each preceded by a comma: lesions_connectivity, lesions_max, lesions_a, hit_a,
// multi_a, lesions_b, hit_b, multi_b, lesion_sensitivity, lesion_precision, lesion_f1, a_lesions and b_lesions
// (arrays of objects: voxels, first, overlap_vox, partners_reported, overlap_other_vox, multi, best,
// best_overlap_vox, coverage, best_dice).
std::string lesions_json_keys(const VolumeCompareLesions& l);
// comparisons.csv: the nine per-volume columns (the six totals and the three derived values), with a leading comma.
std::string lesions_csv_header_fields();
std::string lesions_csv_fields(const VolumeCompareLesions& l);
// compare_lesions.csv: the header line (no newline) and one patient's rows ("\n" after each), side a before b.
std::string lesions_table_header();
std::string lesions_table_rows(const std::string& patient, const VolumeCompareLesions& l);

}  // namespace compare

namespace golden {

// Flood fills of both masks, plain loops over voxels for the pair counts, a std::sort for the order. `a`, `b`:
// w · h · d bytes, non-zero = set.
VolumeCompareLesions compare_volume_lesions(const std::vector<uint8_t>& a, const std::vector<uint8_t>& b, int w, int h, int d,
                                            int max_lesions, int connectivity);

}  // namespace golden
}  // namespace nm03
