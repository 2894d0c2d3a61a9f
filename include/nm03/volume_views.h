// nm03/volume_views.h — the six views of a volume that use its third axis (--volume-views, K14): the
// axial, coronal and sagittal plane through a point P and the maximum-intensity projection along z, y
// and x, each as a plane of stored samples plus a plane of mask bits.
//
//   index  name            content              image (width × height)   spacing (u, v)
//   0      view_axial      plane z = P.z        w × h, row = y           sx, sy
//   1      view_coronal    plane y = P.y        w × d, row = z           sx, sz
//   2      view_sagittal   plane x = P.x        h × d, column = y, row = z   sy, sz
//   3      mip_axial       projection along z   w × h                    sx, sy
//   4      mip_coronal     projection along y   w × d                    sx, sz
//   5      mip_sagittal    projection along x   h × d                    sy, sz
//
// Rows and columns are in index order (plane 0 is the top row of a coronal or sagittal view); the
// orientation of the patient is not consulted.
//
// A projection takes, per pixel, the sample that is largest AS DISPLAYED: the largest key along the axis
// (key_from_raw, pixel_math.h: the value masked to the stored bits, sign bit flipped for signed data — the
// key of nm03/intensity_core.h), or the smallest key when the modality rescale is applied with a negative
// slope (`inverted`). The pixel is the canonical stored sample of the winning key (unsigned: the key;
// signed: the key with its sign bit flipped back, a sign-extended 16-bit value), so a projection has the
// volume's sample format and the raw-gray render applies unchanged. Rescaling x · slope + intercept in f32
// is monotone (non-decreasing for slope > 0, non-increasing for slope < 0), so the maximum of the rescaled
// floats is the rescaled value of that key: both definitions render equal pixels.
// The mask of a plane view is the dilated mask on that plane, of a projection the OR of the dilated mask
// along the axis (its shadow).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "nm03/common.h"
#include "nm03/params.h"
#include "nm03/pixel_math.h"

namespace nm03 {

constexpr int kVolumeViewCount = 6;

// Where the three planes meet (--volume-views-at).
enum ViewsAtMode : int { kViewsAtMask = 0, kViewsAtCentre = 1, kViewsAtPoint = 2 };
struct ViewsAt {
  int mode = kViewsAtMask;
  int x = 0, y = 0, z = 0;  // kViewsAtPoint only
};

struct VolumeView {
  int w = 0, h = 0;
  std::vector<uint16_t> raw;  // h × w stored samples
  std::vector<uint8_t> mask;  // h × w, 0/1
  int32_t raw_min = 0, raw_max = 0;  // stored sample values (stored_sample) of the smallest / largest key
  uint32_t mask_px = 0;
};

struct VolumeViews {
  int w = 0, h = 0, d = 0;
  int at_mode = kViewsAtMask;  // as asked for (a `mask` request on an empty mask keeps its name)
  int at[3] = {0, 0, 0};       // P
  bool has_box = false;        // false: the dilated mask is empty
  int box[6] = {0, 0, 0, 0, 0, 0};  // x0, y0, z0, x1, y1, z1 (inclusive)
  bool inverted = false;
  VolumeView view[kVolumeViewCount];
};

namespace views {

NM03_HD int view_width(int i, int w, int h) { return (i % 3) == 2 ? h : w; }
NM03_HD int view_height(int i, int h, int d) { return (i % 3) == 0 ? h : d; }
const char* view_name(int i);     // "view_axial" … "mip_sagittal"
const char* at_mode_name(int m);  // "mask" | "centre" | "point"
// (u, v) of view i from the volume's spacing; sz is cast to float, as make_render_geom takes it.
void view_spacing(int i, float sx, float sy, double sz, float* u, float* v);
// "mask" | "centre" | "X,Y,Z" (three non-negative decimal integers) → *at; false when `s` is none of them.
bool parse_at(const std::string& s, ViewsAt* at);
// Empty, or why `at` cannot be used for a w × h × d volume (an explicit point outside it: names the
// point and the extent).
std::string at_error(const ViewsAt& at, int w, int h, int d);
// P from the request and the box of the mask (integer division): `mask` gives the centre of the box,
// or the centre of the volume when there is none.
NM03_HD void resolve_at(int mode, int px, int py, int pz, bool has_box, const int* box, int w, int h, int d, int* at) {
  if (mode == kViewsAtPoint) {
    at[0] = px, at[1] = py, at[2] = pz;
  } else if (mode == kViewsAtMask && has_box) {
    at[0] = (box[0] + box[3]) / 2, at[1] = (box[1] + box[4]) / 2, at[2] = (box[2] + box[5]) / 2;
  } else {
    at[0] = w / 2, at[1] = h / 2, at[2] = d / 2;
  }
}
// The canonical stored sample of a key (see the head of this file).
NM03_HD uint16_t sample_of_key(uint16_t key, uint8_t type) { return (uint16_t)(key ^ (type == kI16 ? 0x8000u : 0u)); }

// The sidecar <patient>/views.json: one JSON object on one line (no newline), keys in fixed order — width,
// height, depth, at_mode, at [x, y, z], mask_bbox [x0, y0, z0, x1, y1, z1] or null, inverted, spacing
// [sx, sy, sz], views: six objects in index order with name, width, height, spacing [u, v], raw_min,
// raw_max, mask_px. Doubles as %.9g. The one writer of the GPU path, --cpu and Python.
std::string to_json(const VolumeViews& v, float sx, float sy, double sz);
constexpr const char* kSidecarName = "views.json";
// File names of the twelve JPEGs, in the order of the files the export functions return: per view the
// original, then the processed image.
std::string file_name(int view, bool processed);

}  // namespace views

namespace golden {

// The views of a d × h × w volume of stored samples `raw` and its dilated mask (0/1 per voxel), plain
// loops. `inverted`: the smallest key wins a projection. Throws std::invalid_argument for an `at` that
// views::at_error refuses.
VolumeViews volume_views(const uint16_t* raw, const uint8_t* dilated, int w, int h, int d, uint8_t type, int stored_bits,
                         bool inverted, const ViewsAt& at);
// The twelve files of `v` (views::file_name order): every gray view windowed by the min / max of its own
// rescaled pixels, labels with the renderer border of the view's own 2D image, on the rp.out_width ×
// rp.out_height canvas at the view's spacing. slope / intercept: as applied (1, 0 without apply_rescale).
std::vector<std::vector<uint8_t>> volume_view_jpegs(const VolumeViews& v, uint8_t type, int stored_bits, float slope,
                                                    float intercept, float sx, float sy, double sz, const RenderParams& rp);

}  // namespace golden

}  // namespace nm03
