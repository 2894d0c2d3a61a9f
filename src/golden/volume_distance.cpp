// The exact Euclidean distance map of a volume mask in physical space (nm03/volume_distance.h): the golden
// model (whole-line minima, a direct margin, plain thickness loops), the host run of the K16 kernels'
// per-line functions and the one writer of the sidecar keys.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "nm03/volume_distance.h"
#include "nm03/volume_distance_core.h"

namespace nm03 {

namespace {

void check_args(const char* who, int w, int h, int d, const uint32_t um[3]) {
  if (w < 1 || h < 1 || d < 1) throw std::invalid_argument(std::string(who) + ": empty volume");
  if (w > 65535) throw std::invalid_argument(std::string(who) + ": a row holds at most 65535 voxels");
  for (int a = 0; a < 3; ++a)
    if (um[a] < 1u) throw std::invalid_argument(std::string(who) + ": a spacing must be at least 1 um");
  const std::string ext = measure::volume_distance_extent_error(w, h, d, um);
  if (!ext.empty()) throw std::invalid_argument(std::string(who) + ": " + ext);
}

int64_t cap_squared(int64_t cap_um) {
  if (cap_um < 0) return -1;
  return cap_um >= (1ll << 31) ? (1ll << 62) : cap_um * cap_um;  // the extent rule keeps every distance below 2^62
}

std::string u128_text(unsigned __int128 v) {
  std::string s;
  do s.insert(s.begin(), (char)('0' + (int)(v % 10))), v /= 10;
  while (v);
  return s;
}

}  // namespace

namespace measure {

std::string volume_distance_extent_error(int w, int h, int d, const uint32_t um[3]) {
  const int dim[3] = {w, h, d};
  unsigned __int128 sum = 0;
  for (int a = 0; a < 3; ++a) {
    const unsigned __int128 e = (unsigned __int128)(uint64_t)std::max(0, dim[a] - 1) * um[a];
    sum += e * e;  // < 3 · 2^126: no wrap
  }
  if (sum < ((unsigned __int128)1 << 62)) return std::string();
  return "the volume is too long for a distance map in micrometres: ((w - 1) * ux)^2 + ((h - 1) * uy)^2 + ((d - 1) * uz)^2 = " +
         u128_text(sum) + " must stay below 2^62";
}

int64_t dilate_mm_to_um(double mm) { return (int64_t)std::llround(mm * 1000.0); }

void volume_distance_words(const uint64_t* bits, int w, int h, int d, int wpr, const uint32_t um[3], bool to_background,
                           int64_t cap_um, int64_t* out) {
  check_args("volume_distance_words", w, h, d, um);
  if (wpr != (w + 63) / 64) throw std::invalid_argument("volume_distance_words: wpr must be ceil(w / 64)");
  using namespace vdist;
  const int64_t cap2 = cap_squared(cap_um);
  const size_t n = (size_t)w * h * d, plane = (size_t)w * h;
  std::vector<uint16_t> g(n);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y) {
      const uint64_t* row = bits + ((size_t)z * h + y) * wpr;
      for (int kw = 0; kw < wpr; ++kw) {  // a wave of the rows kernel
        const uint64_t s = set_word(row, kw, w, to_background);
        const int32_t left = left_reach(row, w, to_background, kw), right = right_reach(row, wpr, w, to_background, kw);
        for (int b = 0; b < 64 && kw * 64 + b < w; ++b) g[((size_t)z * h + y) * w + kw * 64 + b] = row_distance(s, b, left, right);
      }
    }
  std::vector<int64_t> c(n);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const uint16_t* col = g.data() + (size_t)z * plane + x;
        c[(size_t)z * plane + (size_t)y * w + x] =
            capped(search_line(h, y, um[1], cap2, [&](int j) { return row_value(col[(size_t)j * w], um[0]); }), cap2);
      }
  for (int z = 0; z < d; ++z)
    for (size_t i = 0; i < plane; ++i)
      out[(size_t)z * plane + i] = capped(search_line(d, z, um[2], cap2, [&](int j) { return c[(size_t)j * plane + i]; }), cap2);
}

VolumeThickness volume_thickness_words(const uint64_t* bits, int w, int h, int d, int wpr, const uint32_t um[3]) {
  check_args("volume_thickness_words", w, h, d, um);
  std::vector<int64_t> D((size_t)w * h * d);
  volume_distance_words(bits, w, h, d, wpr, um, true, -1, D.data());
  int64_t bv = 0;
  uint64_t bp = vdist::kNoCandidate;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const uint64_t p = ((uint64_t)z * h + y) * w + x;
        const bool in_mask = (bits[((size_t)z * h + y) * wpr + (x >> 6)] >> (x & 63)) & 1ull;
        if (in_mask && D[p] != kNoDistance && vdist::better(D[p], p, bv, bp)) bv = D[p], bp = p;
      }
  VolumeThickness t{};
  t.at[0] = t.at[1] = t.at[2] = -1;
  if (bp != vdist::kNoCandidate) {
    t.inscribed_um2 = (uint64_t)bv;
    t.at[0] = (int32_t)(bp % (uint64_t)w), t.at[1] = (int32_t)(bp / (uint64_t)w % (uint64_t)h), t.at[2] = (int32_t)(bp / ((uint64_t)w * h));
    t.found = 1;
  }
  return t;
}

double inscribed_radius_mm(const VolumeThickness& t) { return t.found ? std::sqrt((double)t.inscribed_um2) / 1000.0 : 0.0; }

std::string thickness_keys(const VolumeThickness& t, const uint32_t um[3]) {
  char buf[512];
  int n = std::snprintf(buf, sizeof buf, ",\"thickness_spacing_um\":[%u,%u,%u],\"inscribed_um2\":%llu,\"inscribed_at\":[%d,%d,%d]", um[0],
                        um[1], um[2], (unsigned long long)t.inscribed_um2, t.at[0], t.at[1], t.at[2]);
  if (t.found) {
    const double r = inscribed_radius_mm(t);
    std::snprintf(buf + n, sizeof buf - n, ",\"inscribed_radius_mm\":%.9g,\"thickness_mm\":%.9g", r, 2.0 * r);
  } else {
    std::snprintf(buf + n, sizeof buf - n, ",\"inscribed_radius_mm\":null,\"thickness_mm\":null");
  }
  return buf;
}

std::string insert_thickness_keys(std::string text, const VolumeThickness& t, const uint32_t um[3]) {
  size_t at = text.find(",\"diameters_spacing_um\":");
  if (at == std::string::npos) at = text.find(",\"lesions_max\":");
  if (at == std::string::npos) {
    if (text.size() < 2) throw std::invalid_argument("insert_thickness_keys: not a sidecar text");
    at = text.size() - 2;  // the text ends with "}\n"
  }
  text.insert(at, thickness_keys(t, um));
  return text;
}

}  // namespace measure

namespace golden {

std::vector<int64_t> volume_distance(const std::vector<uint8_t>& mask, int w, int h, int d, const uint32_t um[3],
                                     bool to_background, int64_t cap_um) {
  check_args("golden::volume_distance", w, h, d, um);
  const size_t n = (size_t)w * h * d, plane = (size_t)w * h;
  if (mask.size() != n) throw std::invalid_argument("golden::volume_distance: the mask must hold w * h * d voxels");
  const int64_t cap2 = cap_squared(cap_um);
  auto sq = [](int64_t steps, uint32_t u) {
    const int64_t v = steps * (int64_t)u;
    return v * v;
  };
  std::vector<int64_t> a(n), b(n);
  for (size_t i = 0; i < n; ++i) a[i] = ((mask[i] != 0) != to_background) ? 0 : kNoDistance;
  // one pass: b(i) = min over the whole line of a(j) + ((i − j)·u)²
  auto pass = [&](int len, size_t stride, uint32_t u, size_t lines_outer, size_t outer_stride, size_t lines_inner, size_t inner_stride) {
    for (size_t o = 0; o < lines_outer; ++o)
      for (size_t q = 0; q < lines_inner; ++q) {
        const size_t base = o * outer_stride + q * inner_stride;
        for (int i = 0; i < len; ++i) {
          int64_t best = kNoDistance;
          for (int j = 0; j < len; ++j) {
            const int64_t v = a[base + (size_t)j * stride];
            if (v == kNoDistance) continue;
            best = std::min(best, v + sq(i - j, u));
          }
          b[base + (size_t)i * stride] = best;
        }
      }
    a.swap(b);
  };
  pass(w, 1, um[0], (size_t)d, plane, (size_t)h, (size_t)w);
  pass(h, (size_t)w, um[1], (size_t)d, plane, (size_t)w, 1);
  pass(d, plane, um[2], (size_t)h, (size_t)w, (size_t)w, 1);
  if (cap2 >= 0)
    for (int64_t& v : a)
      if (v > cap2) v = kNoDistance;
  return a;
}

std::vector<uint8_t> dilate3d_mm(const std::vector<uint8_t>& region, int w, int h, int d, const uint32_t um[3], int64_t r_um) {
  check_args("golden::dilate3d_mm", w, h, d, um);
  if (r_um < 0) throw std::invalid_argument("golden::dilate3d_mm: the radius must not be negative");
  const size_t n = (size_t)w * h * d, plane = (size_t)w * h;
  if (region.size() != n) throw std::invalid_argument("golden::dilate3d_mm: the region must hold w * h * d voxels");
  const int64_t r2 = cap_squared(r_um);
  struct Off {
    int dx, dy, dz;
  };
  std::vector<Off> offs;
  const int mx = (int)std::min<int64_t>(w - 1, r_um / um[0]), my = (int)std::min<int64_t>(h - 1, r_um / um[1]),
            mz = (int)std::min<int64_t>(d - 1, r_um / um[2]);
  for (int dz = -mz; dz <= mz; ++dz)
    for (int dy = -my; dy <= my; ++dy)
      for (int dx = -mx; dx <= mx; ++dx) {
        const int64_t ex = (int64_t)dx * um[0], ey = (int64_t)dy * um[1], ez = (int64_t)dz * um[2];
        if (ex * ex + ey * ey + ez * ez <= r2) offs.push_back({dx, dy, dz});
      }
  std::vector<uint8_t> out(n, 0);
  auto set_at = [&](int x, int y, int z) { return x >= 0 && x < w && y >= 0 && y < h && z >= 0 && z < d && region[(size_t)z * plane + (size_t)y * w + x]; };
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        if (!region[(size_t)z * plane + (size_t)y * w + x]) continue;
        out[(size_t)z * plane + (size_t)y * w + x] = 1;
        // a voxel whose six face neighbours are all set adds nothing its neighbours do not add
        if (set_at(x - 1, y, z) && set_at(x + 1, y, z) && set_at(x, y - 1, z) && set_at(x, y + 1, z) && set_at(x, y, z - 1) &&
            set_at(x, y, z + 1))
          continue;
        for (const Off& o : offs) {
          const int xx = x + o.dx, yy = y + o.dy, zz = z + o.dz;
          if (xx >= 0 && xx < w && yy >= 0 && yy < h && zz >= 0 && zz < d) out[(size_t)zz * plane + (size_t)yy * w + xx] = 1;
        }
      }
  return out;
}

VolumeThickness volume_thickness(const std::vector<uint8_t>& mask, int w, int h, int d, const uint32_t um[3]) {
  const std::vector<int64_t> D = volume_distance(mask, w, h, d, um, true, -1);
  VolumeThickness t{};
  t.at[0] = t.at[1] = t.at[2] = -1;
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t p = ((size_t)z * h + y) * w + x;
        if (!mask[p] || D[p] == kNoDistance) continue;
        if (!t.found || (uint64_t)D[p] > t.inscribed_um2) {  // raster order: the first one at the maximum stays
          t.inscribed_um2 = (uint64_t)D[p];
          t.at[0] = x, t.at[1] = y, t.at[2] = z;
          t.found = 1;
        }
      }
  return t;
}

}  // namespace golden
}  // namespace nm03
