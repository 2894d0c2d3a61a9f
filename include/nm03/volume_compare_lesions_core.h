// nm03/volume_compare_lesions_core.h — what one thread of the K18 kernels (src/kernels/k18_volume_compare_lesions.hip)
// does for its word of the two bit volumes, as host/device functions. measure::volume_compare_lesions_words runs
// exactly these on the host, a word after the other, so the stretch walk of the join, the partner-cell transition,
// the rank lookup and the best partner with its tie rule are checked without a GPU. The labelling itself is K8's
// (nm03/volume_measure_core.h).
//
// SIDE DATA of a mask: one u32 array of K8's slot layout next to its labelling. For a root at slot s, side[s] is the
// overlap counter (voxels of the component inside the other mask) and side[s + 1] the partner cell — free for the
// same reason K8's area slot is: the voxel right of a run's first voxel never starts a run. The partner cell holds
// 0 = no partner, a partner's root slot + 1, or kSeveral = at least two different partners.
//
// S (side data) provides: uint32_t ld(i), void st(i, v), void add(i, v), uint32_t cas(i, expected, desired) (returns
// the old value).
#pragma once

#include <cstdint>

#include "nm03/measure.h"
#include "nm03/volume_compare_lesions.h"
#include "nm03/volume_measure_core.h"

namespace nm03::vclcore {

constexpr uint32_t kSeveral = 0xFFFFFFFFu;  // no slot + 1 reaches it: (w + 1)·h·d + 1 fits 32 bits

// The partner cell after meeting the partner at root slot `slot`.
NM03_HD uint32_t partner_next(uint32_t cell, uint32_t slot) {
  const uint32_t v = slot + 1u;
  return cell == 0u ? v : (cell == v || cell == kSeveral) ? cell : kSeveral;
}

// Applies the transition at side[root + 1]. A cell changes at most twice (0 → one partner → several), so the loop
// takes at most three trips; a cell that already says what the partner would make it is only read.
template <class S>
NM03_HD void partner_update(S& side, uint32_t root, uint32_t partner) {
  uint32_t cur = side.ld(root + 1u);
  for (;;) {
    const uint32_t next = partner_next(cur, partner);
    if (next == cur) return;
    const uint32_t old = side.cas(root + 1u, cur, next);
    if (old == cur) return;
    cur = old;
  }
}

// The side data of every root among the runs that start in word (z, y, k): counter 0, no partner.
template <class P, class S>
NM03_HD void init_side(const vmcore::BitVolume& V, P& par, S& side, int z, int y, int k) {
  for (uint64_t t = vmcore::root_bits(V, par, z, y, k); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + vmcore::ctz64(t));
    side.st(s, 0u);
    side.st(s + 1u, 0u);
  }
}

// Every in-word stretch of A ∧ B in word (z, y, k): emit(root of A's run, root of B's run, length). Such a stretch
// lies in exactly one run of each mask; either run may have started in an earlier word (BitVolume::run_start walks
// left). Both labellings have their runs pointed at their roots (vmcore::compress_runs).
template <class PA, class PB, class Emit>
NM03_HD void join_stretches(const vmcore::BitVolume& A, const vmcore::BitVolume& B, PA& para, PB& parb, int z, int y, int k, Emit&& emit) {
  const uint64_t m = A.at(z, y, k) & B.at(z, y, k);
  for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {
    const int b = vmcore::ctz64(t);
    const uint64_t rest = ~(m >> b);  // bit j clear while voxel b + j is set
    const uint32_t len = rest == 0ull ? 64u - (uint32_t)b : (uint32_t)vmcore::ctz64(rest);
    const int x = (k << 6) + b;
    emit(vmcore::compressed_root(para, A.run_slot(z, y, x)), vmcore::compressed_root(parb, B.run_slot(z, y, x)), len);
  }
}

// The rank of the component at `root` among the reported ones (srt_slot ascending, srt_rank their ranks), or
// `none` (= N, the index that collects the unreported components).
NM03_HD int lesion_rank(const uint32_t* srt_slot, const uint32_t* srt_rank, int count, uint32_t root, int none) {
  const int i = vmcore::find_slot(srt_slot, count, root);
  return i < 0 ? none : (int)srt_rank[i];
}

// The roots among the runs that start in word (z, y, k): their count, those with an overlap and those with several
// partners.
template <class P, class S>
NM03_HD void count_side(const vmcore::BitVolume& V, P& par, S& side, int z, int y, int k, uint32_t& lesions, uint32_t& hit,
                        uint32_t& multi) {
  for (uint64_t t = vmcore::root_bits(V, par, z, y, k); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + vmcore::ctz64(t));
    ++lesions;
    hit += side.ld(s) != 0u;
    multi += side.ld(s + 1u) == kSeveral;
  }
}

// The best partner among cells line[0], line[stride], … (count of them): the largest, a tie to the smaller index;
// −1 when every cell is 0. `partners` receives the number of non-zero cells, `best_overlap` the best cell.
NM03_HD int best_partner(const uint64_t* line, int stride, int count, uint32_t& partners, uint64_t& best_overlap) {
  int best = -1;
  partners = 0u;
  best_overlap = 0ull;
  for (int j = 0; j < count; ++j) {
    const uint64_t v = line[(size_t)j * (size_t)stride];
    partners += v != 0ull;
    if (v > best_overlap) best_overlap = v, best = j;
  }
  return best;
}

// The record of a reported lesion: root slot, voxel count, its side data and its line of the table (row for A with
// stride 1, column for B with stride N + 1); `others` = the other side's reported count, `none` = N.
NM03_HD VolumeCompareLesion lesion_record(const vmcore::BitVolume& V, uint32_t slot, uint32_t voxels, uint32_t overlap, uint32_t partner_cell,
                                          const uint64_t* line, int stride, int others, int none) {
  VolumeCompareLesion r;
  r.voxels = voxels;
  r.overlap_vox = overlap;
  r.overlap_other_vox = line[(size_t)none * (size_t)stride];
  vmcore::slot_voxel(V, slot, r.first);
  r.best = best_partner(line, stride, others, r.partners_reported, r.best_overlap_vox);
  r.multi = partner_cell == kSeveral ? 1 : 0;
  return r;
}

}  // namespace nm03::vclcore
