// nm03/volume_measure_core.h — what one thread of the K8 kernels (src/kernels/k8_volume_measure.hip)
// does for its word of the bit volume, as host/device functions over a parent store `P`. The kernels
// pass relaxed agent-scope atomics on the device scratch; measure::volume_words passes plain accesses
// to a host array and walks the words one after the other, so the word arithmetic, the contact
// stretches and the union-find are checked without a GPU.
//
// The volume is d planes of h rows of n = ceil(w / 64) u64 words (LSB = left-most voxel). The nodes of
// the union-find are the HORIZONTAL RUNS, named by the slot of their first voxel in a layout of w + 1
// slots per row: slot(x, y, z) = (z·h + y)·(w + 1) + x. A run's parent sits at its slot, its area (or,
// in the complement pass, its frame mark) one slot further — free, because the voxel right of a run's
// first voxel never starts a run.
//
// P provides: uint32_t ld(i), void st(i, v), uint32_t fetch_min(i, v) (returns the old value),
// void add(i, v).
#pragma once

#include <cstdint>

#include "nm03/measure.h"

namespace nm03::vmcore {

NM03_HD int ctz64(uint64_t v) { return __builtin_ctzll(v); }
NM03_HD int clz64(uint64_t v) { return __builtin_clzll(v); }
NM03_HD int pop64(uint64_t v) { return __builtin_popcountll(v); }

// Σ of the positions of the set bits of m: six masked popcounts (bit j of the position).
NM03_HD uint32_t bit_position_sum(uint64_t m) {
  return (uint32_t)pop64(m & 0xAAAAAAAAAAAAAAAAull) + 2u * (uint32_t)pop64(m & 0xCCCCCCCCCCCCCCCCull) +
         4u * (uint32_t)pop64(m & 0xF0F0F0F0F0F0F0F0ull) + 8u * (uint32_t)pop64(m & 0xFF00FF00FF00FF00ull) +
         16u * (uint32_t)pop64(m & 0xFFFF0000FFFF0000ull) + 32u * (uint32_t)pop64(m & 0xFFFFFFFF00000000ull);
}

// A bit volume, or (inv) its complement inside the frame: word (z, y, k) masked to the width, 0 outside.
struct BitVolume {
  const uint64_t* p;
  int w, h, d, n;
  bool inv;
  NM03_HD uint64_t at(int z, int y, int k) const {
    if (z < 0 || z >= d || y < 0 || y >= h || k < 0 || k >= n) return 0ull;
    const uint64_t v = p[((size_t)z * (size_t)h + (size_t)y) * (size_t)n + (size_t)k];
    return (inv ? ~v : v) & row_word_mask(k, w);
  }
  NM03_HD uint32_t slot(int z, int y, int x) const {
    return ((uint32_t)z * (uint32_t)h + (uint32_t)y) * ((uint32_t)w + 1u) + (uint32_t)x;
  }
  // Column of the first voxel of the run that contains the set voxel (x, y, z): the position after the
  // highest clear bit below x, walking left through full words (at most n of them).
  NM03_HD int run_start(int z, int y, int x) const {
    int k = x >> 6;
    const int b = x & 63;
    uint64_t c = ~at(z, y, k) & ((b == 63) ? ~0ull : ((2ull << b) - 1ull));
    while (c == 0ull && k > 0) {
      --k;
      c = ~at(z, y, k);
    }
    return c == 0ull ? 0 : (k << 6) + 64 - clz64(c);
  }
  NM03_HD uint32_t run_slot(int z, int y, int x) const { return slot(z, y, run_start(z, y, x)); }
};

// ---- phase A: the figures of one word -----------------------------------------------------------
struct WordFigures {
  uint64_t vox = 0, region = 0, sum_x = 0, sum_y = 0, sum_z = 0, faces_x = 0, faces_y = 0, faces_z = 0;
  EulerCounts e;
  int32_t x0 = 0x7FFFFFFF, y0 = 0x7FFFFFFF, z0 = 0x7FFFFFFF, x1 = -1, y1 = -1, z1 = -1;
};

// The Euler windows at position (y, z) of word k; y = h and z = d are the padding row and plane.
NM03_HD void euler_at(const BitVolume& V, int z, int y, int k, bool all, EulerCounts& e) {
  const uint64_t cur[4] = {V.at(z, y, k), V.at(z, y - 1, k), V.at(z - 1, y, k), V.at(z - 1, y - 1, k)};
  const uint64_t prev[4] = {V.at(z, y, k - 1), V.at(z, y - 1, k - 1), V.at(z - 1, y, k - 1), V.at(z - 1, y - 1, k - 1)};
  euler_word(all, cur, prev, k == V.n - 1 && (V.w & 63) == 0, e);
}

// Adds word (z, y, k)'s share of every figure to `f` and returns the word (for the intensity walk).
// `all`: the Euler windows count when all their voxels are set (6-connectivity), else when any is.
NM03_HD uint64_t word_figures(const BitVolume& V, const uint64_t* region, int z, int y, int k, bool all, WordFigures& f) {
  const uint64_t m = V.at(z, y, k);
  f.region += (uint64_t)pop64(region[((size_t)z * (size_t)V.h + (size_t)y) * (size_t)V.n + (size_t)k] & row_word_mask(k, V.w));
  // This word's windows, and those of the padding row / plane / edge behind the last row and plane.
  euler_at(V, z, y, k, all, f.e);
  if (y == V.h - 1) euler_at(V, z, V.h, k, all, f.e);
  if (z == V.d - 1) euler_at(V, V.d, y, k, all, f.e);
  if (y == V.h - 1 && z == V.d - 1) euler_at(V, V.d, V.h, k, all, f.e);
  if (m == 0ull) return m;
  const uint64_t ml = V.at(z, y, k - 1), mr = V.at(z, y, k + 1);
  const uint32_t c = (uint32_t)pop64(m);
  f.vox += c;
  f.sum_x += (uint64_t)c * (uint32_t)(k << 6) + bit_position_sum(m);
  f.sum_y += (uint64_t)c * (uint32_t)y;
  f.sum_z += (uint64_t)c * (uint32_t)z;
  const int lo = (k << 6) + ctz64(m), hi = (k << 6) + 63 - clz64(m);
  f.x0 = lo < f.x0 ? lo : f.x0;
  f.x1 = hi > f.x1 ? hi : f.x1;
  f.y0 = y < f.y0 ? y : f.y0;
  f.y1 = y > f.y1 ? y : f.y1;
  f.z0 = z < f.z0 ? z : f.z0;
  f.z1 = z > f.z1 ? z : f.z1;
  f.faces_x += (uint64_t)(pop64(m & ~((m << 1) | (ml >> 63))) + pop64(m & ~((m >> 1) | (mr << 63))));
  f.faces_y += (uint64_t)(pop64(m & ~V.at(z, y - 1, k)) + pop64(m & ~V.at(z, y + 1, k)));
  f.faces_z += (uint64_t)(pop64(m & ~V.at(z - 1, y, k)) + pop64(m & ~V.at(z + 1, y, k)));
  return m;
}

// Every run that starts in word (z, y, k): parent = itself, second slot (area / mark) = 0.
template <class P>
NM03_HD void init_runs(const BitVolume& V, int z, int y, int k, P& par) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return;
  const uint64_t ml = V.at(z, y, k - 1);
  for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + ctz64(t));
    par.st(s, s);
    par.st(s + 1, 0u);
  }
}

// ---- phase B: unions ------------------------------------------------------------------------------
// Root of x, halving the path on the way: a node passed over is pointed at its grandparent with a
// fetch_min whose result is not used, so parents only ever decrease and stay ancestors.
template <class P>
NM03_HD uint32_t find_root(P& par, uint32_t x) {
  uint32_t p = par.ld(x);
  while (p != x) {  // parents are strictly smaller than their children: at most x steps
    const uint32_t g = par.ld(p);
    if (g != p) (void)par.fetch_min(x, g);
    x = p;
    p = g;
  }
  return x;
}

// Union of the runs a and b. After a failed fetch_min (another thread lowered the parent of `a`
// first, to `old` < a) the link a → old stands or has been replaced by a → b; either way joining old
// and b restores what is owed, and max(a, b) has strictly decreased: the loop ends.
template <class P>
NM03_HD void unite(P& par, uint32_t a, uint32_t b) {
  for (;;) {
    a = find_root(par, a);
    b = find_root(par, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    const uint32_t old = par.fetch_min(a, b);
    if (old == a) return;
    a = old;
  }
}

// The contacts of word (z, y, k), `m`, with the neighbour row (zr, yr): one union per stretch of
// contact. Straight contacts: the first bit of every stretch of m & a (a stretch lies in one run of
// each row); a stretch that continues from word k − 1 belongs to that word's thread. `wide` (the rows
// also touch at x ± 1): voxel x touching (x − 1) of the other row is owed a union only when neither
// the other row's voxel x nor this row's voxel x − 1 is set — either one already links the two runs
// through a straight contact or by being the same run; x + 1 alike.
template <class P>
NM03_HD void unite_row(const BitVolume& V, P& par, int z, int y, int k, uint64_t m, int zr, int yr, bool wide) {
  if (zr < 0 || yr < 0 || yr >= V.h) return;
  const uint64_t a = V.at(zr, yr, k), ml = V.at(z, y, k - 1), al = V.at(zr, yr, k - 1);
  const int xb = k << 6;
  const uint64_t v = m & a;
  for (uint64_t t = v & ~((v << 1) | ((ml & al) >> 63)); t; t &= t - 1) {
    const int x = xb + ctz64(t);
    unite(par, V.run_slot(z, y, x), V.run_slot(zr, yr, x));
  }
  if (!wide) return;
  const uint64_t mr = V.at(z, y, k + 1), ar = V.at(zr, yr, k + 1);
  for (uint64_t t = m & ((a << 1) | (al >> 63)) & ~a & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
    const int x = xb + ctz64(t);
    unite(par, V.run_slot(z, y, x), V.run_slot(zr, yr, x - 1));
  }
  for (uint64_t t = m & ((a >> 1) | (ar << 63)) & ~a & ~((m >> 1) | (mr << 63)); t; t &= t - 1) {
    const int x = xb + ctz64(t);
    unite(par, V.run_slot(z, y, x), V.run_slot(zr, yr, x + 1));
  }
}

// Word (z, y, k) against the rows that precede it: (y − 1, z) and plane z − 1. At 6-connectivity
// row (y, z − 1) with equal x; at 26-connectivity rows (y − 1 … y + 1, z − 1) and (y − 1, z), x − 1 … x + 1.
template <class P>
NM03_HD void unite_word(const BitVolume& V, P& par, int z, int y, int k, bool conn26) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return;
  unite_row(V, par, z, y, k, m, z, y - 1, conn26);
  unite_row(V, par, z, y, k, m, z - 1, y, conn26);
  if (conn26) {
    unite_row(V, par, z, y, k, m, z - 1, y - 1, true);
    unite_row(V, par, z, y, k, m, z - 1, y + 1, true);
  }
}

// ---- phases C and D (the forest is final) ---------------------------------------------------------
// Every run that starts in word (z, y, k) is pointed straight at its root, so that the chain is walked
// once per run and the later launches read a run's root with one load (compressed_root). Roots are final; a concurrent find reads the old
// parent or the root, both ancestors, and the stored value is the smallest the slot can hold.
template <class P>
NM03_HD void compress_runs(const BitVolume& V, P& par, int z, int y, int k) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return;
  const uint64_t ml = V.at(z, y, k - 1);
  for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + ctz64(t));
    const uint32_t r = find_root(par, s);
    if (r != s) par.st(s, r);
  }
}

// Root of the run at slot s in a launch AFTER compress_runs': one load of the run's own slot. (A find
// would end by reading the root's slot, which for one large body is a single address every thread of
// the launch reads.)
template <class P>
NM03_HD uint32_t compressed_root(P& par, uint32_t s) {
  return par.ld(s);
}

// Every in-word stretch of word (z, y, k): emit(root of its run, its length). The caller adds the
// length at the root's second slot (the kernel first sums the lengths that share a root in the wave).
template <class P, class Emit>
NM03_HD void stretch_areas(const BitVolume& V, P& par, int z, int y, int k, Emit&& emit) {
  const uint64_t m = V.at(z, y, k);
  for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {
    const int b = ctz64(t);
    const uint64_t rest = ~(m >> b);  // bit j clear while voxel b + j is set
    const uint32_t len = rest == 0ull ? 64u - (uint32_t)b : (uint32_t)ctz64(rest);
    emit(compressed_root(par, V.run_slot(z, y, (k << 6) + b)), len);
  }
}

// Complement pass: every in-word stretch of word (z, y, k) with a voxel on one of the six frame faces:
// emit(root of its run). The caller marks the root (second slot = 1); the kernel lets one lane of the
// wave store for all that share a root — every row of the outer background starts and ends on a face.
template <class P, class Emit>
NM03_HD void frame_stretches(const BitVolume& V, P& par, int z, int y, int k, Emit&& emit) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return;
  uint64_t face = 0ull;
  if (z == 0 || z == V.d - 1 || y == 0 || y == V.h - 1) face = ~0ull;
  if (k == 0) face |= 1ull;
  if (k == V.n - 1) face |= 1ull << ((V.w - 1) & 63);
  for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {
    const int b = ctz64(t);
    const uint64_t rest = ~(m >> b);
    const uint32_t len = rest == 0ull ? 64u - (uint32_t)b : (uint32_t)ctz64(rest);
    const uint64_t stretch = (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << b;
    if (stretch & face) emit(compressed_root(par, V.run_slot(z, y, (k << 6) + b)));
  }
}

// The roots among the runs that start in word (z, y, k): their count, the largest second slot (the
// area) and how many have a second slot of 0 (complement pass: unmarked = a cavity).
template <class P>
NM03_HD void count_roots(const BitVolume& V, P& par, int z, int y, int k, uint32_t& roots, uint32_t& largest,
                         uint32_t& unmarked) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return;
  const uint64_t ml = V.at(z, y, k - 1);
  for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + ctz64(t));
    if (par.ld(s) != s) continue;
    ++roots;
    const uint32_t v = par.ld(s + 1);
    largest = v > largest ? v : largest;
    unmarked += v == 0u;
  }
}

// ---- per-lesion phase (K10): on the MASK pass's final labelling ----------------------------------
// After phases C and D of the mask pass every run's slot holds its root and the slot after a root the
// component's voxel count. A root is the smallest slot of its component (unions link the larger root
// under the smaller), so it names the component's first voxel in raster (z, y, x) order.

// The order of the lesions as one u64, larger = earlier: more voxels, then the smaller root slot.
// Slots are unique, so the keys are a total order; 0 is no key (an area is at least 1).
NM03_HD uint64_t lesion_key(uint32_t area, uint32_t slot) { return ((uint64_t)area << 32) | (uint64_t)(uint32_t)~slot; }
NM03_HD uint32_t lesion_key_slot(uint64_t key) { return ~(uint32_t)key; }
NM03_HD uint32_t lesion_key_area(uint64_t key) { return (uint32_t)(key >> 32); }

// The voxel a slot names.
NM03_HD void slot_voxel(const BitVolume& V, uint32_t slot, int32_t xyz[3]) {
  const uint32_t row = slot / ((uint32_t)V.w + 1u);
  xyz[0] = (int32_t)(slot - row * ((uint32_t)V.w + 1u));
  xyz[2] = (int32_t)(row / (uint32_t)V.h);
  xyz[1] = (int32_t)(row - (uint32_t)xyz[2] * (uint32_t)V.h);
}

// The bits of word (z, y, k) at which a run starts that is a root.
template <class P>
NM03_HD uint64_t root_bits(const BitVolume& V, P& par, int z, int y, int k) {
  const uint64_t m = V.at(z, y, k);
  if (m == 0ull) return 0ull;
  const uint64_t ml = V.at(z, y, k - 1);
  uint64_t roots = 0ull;
  for (uint64_t t = m & ~((m << 1) | (ml >> 63)); t; t &= t - 1) {
    const uint32_t s = V.slot(z, y, (k << 6) + ctz64(t));
    if (par.ld(s) == s) roots |= t & (~t + 1ull);
  }
  return roots;
}

// The largest key among the roots at `bits` of word (z, y, k) and, in `bit`, where it starts; 0 for none.
template <class P>
NM03_HD uint64_t best_root_key(const BitVolume& V, P& par, int z, int y, int k, uint64_t bits, int& bit) {
  uint64_t best = 0ull;
  for (uint64_t t = bits; t; t &= t - 1) {
    const int b = ctz64(t);
    const uint32_t s = V.slot(z, y, (k << 6) + b);
    const uint64_t key = lesion_key(par.ld(s + 1u), s);
    if (key > best) best = key, bit = b;
  }
  return best;
}

// Index of `slot` in the ascending array s[0 .. n), −1 when it is not there: at most 7 probes.
NM03_HD int find_slot(const uint32_t* s, int n, uint32_t slot) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s[mid] < slot) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && s[lo] == slot ? lo : -1;
}

// The voxels of word (z, y, k) with an open face — the neighbour on that side is not mask, or the
// frame — on each of the six sides: the global record's faces, kept as bits so that they can be
// masked to the voxels of one lesion.
struct WordFaces {
  uint64_t xl, xh, yl, yh, zl, zh;
};
NM03_HD WordFaces word_faces(const BitVolume& V, int z, int y, int k, uint64_t m) {
  const uint64_t ml = V.at(z, y, k - 1), mr = V.at(z, y, k + 1);
  WordFaces f;
  f.xl = m & ~((m << 1) | (ml >> 63));
  f.xh = m & ~((m >> 1) | (mr << 63));
  f.yl = m & ~V.at(z, y - 1, k);
  f.yh = m & ~V.at(z, y + 1, k);
  f.zl = m & ~V.at(z - 1, y, k);
  f.zh = m & ~V.at(z + 1, y, k);
  return f;
}

// The figures of a set of voxels of one lesion (the intensities aside).
struct LesionFigures {
  uint64_t vox = 0, sum_x = 0, sum_y = 0, sum_z = 0, faces_x = 0, faces_y = 0, faces_z = 0;
  int32_t x0 = 0x7FFFFFFF, y0 = 0x7FFFFFFF, z0 = 0x7FFFFFFF, x1 = -1, y1 = -1, z1 = -1;
};

// Adds the share of the voxels `s` ≠ 0 of word (z, y, k) — stretches of one lesion — to f.
NM03_HD void lesion_bits_figures(int z, int y, int k, const WordFaces& wf, uint64_t s, LesionFigures& f) {
  const uint32_t c = (uint32_t)pop64(s);
  f.vox += c;
  f.sum_x += (uint64_t)c * (uint32_t)(k << 6) + bit_position_sum(s);
  f.sum_y += (uint64_t)c * (uint32_t)y;
  f.sum_z += (uint64_t)c * (uint32_t)z;
  const int lo = (k << 6) + ctz64(s), hi = (k << 6) + 63 - clz64(s);
  f.x0 = lo < f.x0 ? lo : f.x0;
  f.x1 = hi > f.x1 ? hi : f.x1;
  f.y0 = y < f.y0 ? y : f.y0;
  f.y1 = y > f.y1 ? y : f.y1;
  f.z0 = z < f.z0 ? z : f.z0;
  f.z1 = z > f.z1 ? z : f.z1;
  f.faces_x += (uint64_t)(pop64(s & wf.xl) + pop64(s & wf.xh));
  f.faces_y += (uint64_t)(pop64(s & wf.yl) + pop64(s & wf.yh));
  f.faces_z += (uint64_t)(pop64(s & wf.zl) + pop64(s & wf.zh));
}

// Every in-word stretch of word (z, y, k) = m: emit(root of its run, the stretch's bits).
template <class P, class Emit>
NM03_HD void lesion_stretches(const BitVolume& V, P& par, int z, int y, int k, uint64_t m, Emit&& emit) {
  for (uint64_t t = m & ~(m << 1); t; t &= t - 1) {
    const int b = ctz64(t);
    const uint64_t rest = ~(m >> b);  // bit j clear while voxel b + j is set
    const uint32_t len = rest == 0ull ? 64u - (uint32_t)b : (uint32_t)ctz64(rest);
    const uint64_t bits = (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << b;
    emit(compressed_root(par, V.run_slot(z, y, (k << 6) + b)), bits);
  }
}

}  // namespace nm03::vmcore
