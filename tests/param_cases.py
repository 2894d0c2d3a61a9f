"""Inputs and derived bounds of the non-default-parameter GPU tests (test_gpu_params.py; not a conftest).

Everything here is NumPy on the CPU: the structured SRG band, the label-like and noise canvases, the
sharpen inputs and the error bound of the float32 sharpen against its float64 reference."""
import numpy as np

# ---- K1b sharpen --------------------------------------------------------------------------------
SHARPEN_MASKS = (1, 3, 5, 7, 9, 11, 13, 15)
SHARPEN_DEFAULT = (2.0, 0.5)           # (gain, sigma)
SHARPEN_OTHER = ((0.75, 1.3), (4.0, 3.0))
# 72×136: W % 4 == 0 (vector loads), three tiles per row. 67×131: per-pixel loads, partial tiles in x
# and y. 40×136: one row of three tiles, so the last workgroup has a single tile.
SHARPEN_SHAPES = ((72, 136), (67, 131), (40, 136))


def sharpen_variant(mask, variant):
    """(gain, sigma, srg_min, srg_max) of a sharpen case: the defaults, or the other pair that the
    mask's index selects together with a moved band."""
    if variant == "default":
        return SHARPEN_DEFAULT + (0.74, 0.91)
    return SHARPEN_OTHER[SHARPEN_MASKS.index(mask) % 2] + (0.70, 0.95)


def noise12(h, w, seed):
    """12-bit uniform noise: after the median its normalised values straddle both band edges."""
    return np.random.default_rng(seed).integers(0, 4096, size=(h, w), dtype=np.uint16)


def sharpen_bound(mask, gain, cmax):
    """|float32 sharpen − float64 sharpen| ≤ (2·mask + 4) · 2⁻²⁴ · (1 + 2·|gain|) · max|c|.

    An output is a chain of about 2·mask + 4 float32 roundings: mask taps and mask accumulations per
    pass are fmas (one rounding each, 2·mask for both passes), then c − b, gain·d, c + g and the
    rounding of the taps themselves. Every rounded quantity is bounded by (1 + 2·|gain|)·max|c| (the
    blur b by max|c|, d by 2·max|c|, s by (1 + 2·|gain|)·max|c|), and a rounding of x errs by at most
    2⁻²⁴·|x|; errors made before the combine are amplified by at most 1 + 2·|gain|, which the common
    factor already covers for the terms bounded by max|c|."""
    return (2 * mask + 4) * 2.0 ** -24 * (1 + 2 * abs(gain)) * float(cmax)


def clip_ramp(h, w, lo, hi, seed):
    """Integers in [lo, hi]: a diagonal ramp over the whole range plus ±3 % noise, so that a
    normalise + clip whose window lies inside [lo, hi] clips on both sides and passes values between."""
    y, x = np.mgrid[0:h, 0:w]
    t = (x + y) / float(h + w - 2)
    v = lo + t * (hi - lo) + np.random.default_rng(seed).normal(0, 0.03 * (hi - lo), (h, w))
    return np.clip(np.rint(v), lo, hi).astype(np.int64)


# ---- K2 morphology ------------------------------------------------------------------------------
MORPH_SIZES = ((1, 1), (5, 7), (9, 3), (31, 33), (63, 63))  # (dilation, erosion)
MORPH_SHAPES = ((131, 77), (100, 200))                      # 2 words with a partial last word; 4 words
MORPH_LARGE = (600, 520)                                    # global-memory planes, (5, 7) only
BORDER_RADII = (1, 3, 5)
NOTCH = 66                                                  # > 2·31 + 1: a 63-wide dilation leaves it open


def structured_band(h, w):
    """A solid block with one-pixel holes: set everywhere except
      * a one-pixel background frame along the top row and the left column (the block touches the
        right and bottom image edges, where erosion counts outside as set and dilation as clear);
      * a NOTCH-row × (NOTCH + 1)-column background notch on the left, which the widest dilation
        (63) cannot close, leaving a strip of ≥ 10 columns that joins the parts above and below;
      * a diagonal chain inside the notch that hangs on the block by one pixel: connectivity 8
        follows it, connectivity 4 takes its first pixel only;
      * a handful of one-pixel holes above and below the notch (an erosion wipes a size² square
        around each)."""
    assert h >= NOTCH + 30 and w >= NOTCH + 11
    b = np.ones((h, w), bool)
    b[0, :] = False
    b[:, 0] = False
    ny = (h - NOTCH) // 2
    b[ny:ny + NOTCH, :NOTCH + 1] = False
    for k in range(4):
        b[ny + 3 + k, NOTCH - k] = True
    for y, x in ((3, 5), (2, 10), (ny // 2, w // 2), (5, w - 3), (h - 4, 3), (ny + NOTCH + 2, 12), (ny + 8, w - 4)):
        b[y, x] = False
    return b


# ---- K4 JPEG ------------------------------------------------------------------------------------
JPEG_QUALITIES = (10, 50, 90, 100)
JPEG_EXTRA_QUALITIES = (1, 25, 95)  # golden == Pillow for these too (tests/test_jpeg.py, test_jpeg_rgb.py)


def label_canvas(h, w):
    """Label-like canvas: flat areas of 0 / 153 / 255 with a few edges, most 8×8 blocks one colour."""
    c = np.zeros((h, w), np.uint8)
    c[h // 4: 3 * h // 4, w // 5: 4 * w // 5] = 153
    c[h // 4: 3 * h // 4, w // 5: w // 5 + 2] = 255
    c[h // 4: h // 4 + 2, w // 5: 4 * w // 5] = 255
    c[:, 7 * w // 8:] = 255
    c[h // 2 + 3, :] = 255
    return c


def noise_canvas(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)
