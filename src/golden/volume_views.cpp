// Golden model of the volume views (nm03/volume_views.h): plain loops over the voxels, the sidecar
// writer and the host render + encode of the twelve files. The oracle of the K14 kernels.
#include "nm03/volume_views.h"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

#include "nm03/golden.h"
#include "nm03/jpeg.h"
#include "nm03/measure.h"

namespace nm03 {

namespace views {

const char* view_name(int i) {
  static const char* const names[kVolumeViewCount] = {"view_axial", "view_coronal", "view_sagittal",
                                                      "mip_axial",  "mip_coronal",  "mip_sagittal"};
  return i >= 0 && i < kVolumeViewCount ? names[i] : "";
}

const char* at_mode_name(int m) { return m == kViewsAtMask ? "mask" : m == kViewsAtCentre ? "centre" : "point"; }

void view_spacing(int i, float sx, float sy, double sz, float* u, float* v) {
  *u = (i % 3) == 2 ? sy : sx;
  *v = (i % 3) == 0 ? sy : (float)sz;
}

bool parse_at(const std::string& s, ViewsAt* at) {
  if (s == "mask" || s == "centre") {
    at->mode = s == "mask" ? kViewsAtMask : kViewsAtCentre;
    at->x = at->y = at->z = 0;
    return true;
  }
  int p[3] = {0, 0, 0};
  size_t pos = 0;
  for (int k = 0; k < 3; ++k) {
    size_t end = pos;
    while (end < s.size() && s[end] >= '0' && s[end] <= '9') ++end;
    if (end == pos || end - pos > 9) return false;
    p[k] = std::atoi(s.substr(pos, end - pos).c_str());
    if (k < 2 ? (end >= s.size() || s[end] != ',') : end != s.size()) return false;
    pos = end + 1;
  }
  at->mode = kViewsAtPoint;
  at->x = p[0], at->y = p[1], at->z = p[2];
  return true;
}

std::string at_error(const ViewsAt& at, int w, int h, int d) {
  if (at.mode != kViewsAtMask && at.mode != kViewsAtCentre && at.mode != kViewsAtPoint) return "unknown views-at mode";
  if (at.mode != kViewsAtPoint) return "";
  if (at.x >= 0 && at.y >= 0 && at.z >= 0 && at.x < w && at.y < h && at.z < d) return "";
  return "the point (" + std::to_string(at.x) + ", " + std::to_string(at.y) + ", " + std::to_string(at.z) +
         ") lies outside the volume of " + std::to_string(w) + " x " + std::to_string(h) + " x " + std::to_string(d);
}

std::string file_name(int view, bool processed) {
  return std::string(view_name(view)) + (processed ? "_processed.jpg" : "_original.jpg");
}

std::string to_json(const VolumeViews& v, float sx, float sy, double sz) {
  auto num = [](double x) {
    char b[40];
    std::snprintf(b, sizeof b, "%.9g", x);
    return std::string(b);
  };
  std::string s = "{\"width\":" + std::to_string(v.w) + ",\"height\":" + std::to_string(v.h) +
                  ",\"depth\":" + std::to_string(v.d) + ",\"at_mode\":\"" + at_mode_name(v.at_mode) + "\",\"at\":[" +
                  std::to_string(v.at[0]) + "," + std::to_string(v.at[1]) + "," + std::to_string(v.at[2]) + "],\"mask_bbox\":";
  if (v.has_box) {
    s += "[";
    for (int k = 0; k < 6; ++k) s += (k ? "," : "") + std::to_string(v.box[k]);
    s += "]";
  } else {
    s += "null";
  }
  s += std::string(",\"inverted\":") + (v.inverted ? "true" : "false");
  s += ",\"spacing\":[" + num((double)sx) + "," + num((double)sy) + "," + num(sz) + "],\"views\":[";
  for (int i = 0; i < kVolumeViewCount; ++i) {
    const VolumeView& q = v.view[i];
    // (u, v) as view_spacing gives them, printed from the doubles, so sz keeps its digits
    const double du = (i % 3) == 2 ? (double)sy : (double)sx, dv = (i % 3) == 0 ? (double)sy : sz;
    s += std::string(i ? "," : "") + "{\"name\":\"" + view_name(i) + "\",\"width\":" + std::to_string(q.w) +
         ",\"height\":" + std::to_string(q.h) + ",\"spacing\":[" + num(du) + "," + num(dv) + "],\"raw_min\":" +
         std::to_string(q.raw_min) + ",\"raw_max\":" + std::to_string(q.raw_max) + ",\"mask_px\":" + std::to_string(q.mask_px) +
         "}";
  }
  s += "]}";
  return s;
}

}  // namespace views

namespace golden {

VolumeViews volume_views(const uint16_t* raw, const uint8_t* dilated, int w, int h, int d, uint8_t type, int stored_bits,
                         bool inverted, const ViewsAt& at) {
  if (w < 1 || h < 1 || d < 1) throw std::invalid_argument("volume views: empty volume");
  if (stored_bits < 1 || stored_bits > 16) throw std::invalid_argument("volume views: stored bits must be 1..16");
  const std::string err = views::at_error(at, w, h, d);
  if (!err.empty()) throw std::invalid_argument("volume views: " + err);
  if (type == kU8) type = kU16;  // 8-bit data is held as unsigned 16-bit samples with stored_bits = 8
  VolumeViews r;
  r.w = w, r.h = h, r.d = d;
  r.at_mode = at.mode;
  r.inverted = inverted;
  const size_t plane = (size_t)w * h;
  auto vox = [&](int x, int y, int z) { return (size_t)z * plane + (size_t)y * w + x; };
  // the box of the mask
  int b[6] = {w, h, d, -1, -1, -1};
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        if (dilated[vox(x, y, z)]) {
          b[0] = std::min(b[0], x), b[1] = std::min(b[1], y), b[2] = std::min(b[2], z);
          b[3] = std::max(b[3], x), b[4] = std::max(b[4], y), b[5] = std::max(b[5], z);
        }
  r.has_box = b[3] >= 0;
  if (r.has_box) std::copy(b, b + 6, r.box);
  views::resolve_at(at.mode, at.x, at.y, at.z, r.has_box, r.box, w, h, d, r.at);
  for (int i = 0; i < kVolumeViewCount; ++i) {
    VolumeView& q = r.view[i];
    q.w = views::view_width(i, w, h);
    q.h = views::view_height(i, h, d);
    q.raw.assign((size_t)q.w * q.h, 0);
    q.mask.assign((size_t)q.w * q.h, 0);
  }
  // the three planes through P: the stored samples as they are
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      r.view[0].raw[(size_t)y * w + x] = raw[vox(x, y, r.at[2])];
      r.view[0].mask[(size_t)y * w + x] = dilated[vox(x, y, r.at[2])] ? 1 : 0;
    }
  for (int z = 0; z < d; ++z)
    for (int x = 0; x < w; ++x) {
      r.view[1].raw[(size_t)z * w + x] = raw[vox(x, r.at[1], z)];
      r.view[1].mask[(size_t)z * w + x] = dilated[vox(x, r.at[1], z)] ? 1 : 0;
    }
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y) {
      r.view[2].raw[(size_t)z * h + y] = raw[vox(r.at[0], y, z)];
      r.view[2].mask[(size_t)z * h + y] = dilated[vox(r.at[0], y, z)] ? 1 : 0;
    }
  // the three projections: the winning key per pixel, then its canonical sample
  std::vector<int32_t> best[3];
  best[0].assign(plane, -1);
  best[1].assign((size_t)w * d, -1);
  best[2].assign((size_t)h * d, -1);
  for (int z = 0; z < d; ++z)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const int32_t key = key_from_raw(raw[vox(x, y, z)], type, (uint8_t)stored_bits);
        const size_t pix[3] = {(size_t)y * w + x, (size_t)z * w + x, (size_t)z * h + y};
        for (int a = 0; a < 3; ++a) {
          int32_t& cur = best[a][pix[a]];
          if (cur < 0 || (inverted ? key < cur : key > cur)) cur = key;
          if (dilated[vox(x, y, z)]) r.view[3 + a].mask[pix[a]] = 1;
        }
      }
  for (int a = 0; a < 3; ++a)
    for (size_t i = 0; i < best[a].size(); ++i) r.view[3 + a].raw[i] = views::sample_of_key((uint16_t)best[a][i], type);
  for (int i = 0; i < kVolumeViewCount; ++i) {
    VolumeView& q = r.view[i];
    int32_t lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
    for (uint16_t s : q.raw) {
      const int32_t v = stored_sample(s, type, (uint8_t)stored_bits);
      lo = std::min(lo, v), hi = std::max(hi, v);
    }
    q.raw_min = lo, q.raw_max = hi;
    for (uint8_t m : q.mask) q.mask_px += m;
  }
  return r;
}

std::vector<std::vector<uint8_t>> volume_view_jpegs(const VolumeViews& v, uint8_t type, int stored_bits, float slope,
                                                    float intercept, float sx, float sy, double sz, const RenderParams& rp) {
  if (type == kU8) type = kU16;
  std::vector<std::vector<uint8_t>> files((size_t)2 * kVolumeViewCount);
  for (int i = 0; i < kVolumeViewCount; ++i) {
    const VolumeView& q = v.view[i];
    float su = 1.f, sv = 1.f;
    views::view_spacing(i, sx, sy, sz, &su, &sv);
    const RenderGeom g = make_render_geom(q.w, q.h, su, sv, rp.out_width, rp.out_height);
    std::vector<float> vals(q.raw.size());
    for (size_t k = 0; k < vals.size(); ++k)
      vals[k] = rescaled_value(key_from_raw(q.raw[k], type, (uint8_t)stored_bits), type, slope, intercept);
    const auto mm = std::minmax_element(vals.begin(), vals.end());
    const auto c0 = render_gray(vals, g, *mm.first, *mm.second, rp.filter == kFilterNearest);
    const auto c1 = render_labels(q.mask, border(q.mask, q.w, q.h, rp.border_radius), g, opacity_u8(rp.label_opacity),
                                  opacity_u8(rp.border_opacity));
    files[(size_t)2 * i] = jpeg::encode_gray(c0.data(), rp.out_width, rp.out_height, rp.out_width, rp.jpeg_quality,
                                             (jpeg::Sampling)rp.jpeg_sampling);
    files[(size_t)2 * i + 1] = jpeg::encode_gray(c1.data(), rp.out_width, rp.out_height, rp.out_width, rp.jpeg_quality,
                                                 (jpeg::Sampling)rp.jpeg_sampling);
  }
  return files;
}

}  // namespace golden
}  // namespace nm03
