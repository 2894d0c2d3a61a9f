"""Inputs of the large-slice tests (test_large_slice_cases.py on the CPU, test_gpu_large_slices.py on the
GPU; not a conftest): 2D slices with a side between 1025 and gpu_types.h kMaxSliceDim = 4096, where the
kernels' loops wrap for the first time and the packed fields of K9 and the 32-bit sums of K7 are full.
Everything here is NumPy on the CPU. Shapes are (h, w); each is the smallest that reaches its hazard:

  rows_wrap    (1030, 70)    a K2 thread (1024 per workgroup) owns two rows; 17 words per transposed row
  cols_wrap    (70, 1030)    the K2 column fill and the morphology row loops wrap; 17 words per row, the
                             last one partial (1030 = 16·64 + 6)
  both_wrap    (1100, 1040)  both at once; the mid-size case of the engine end to end
  tall_limit   (4096, 100)   y = 4095; 64 words per transposed row; K9's row arrays to their last entry
  wide_limit   (100, 4096)   x = 4095; 64 full words per row
  sum64        (4096, 600)   Σy of a full mask = 600 · 4095 · 4096 / 2 ≈ 5.03e9 > 2³²
  square_limit (4096, 4096)  all four 12-bit fields of K9's pair key at 0xFFF; d² = 2 · 4095² < 2²⁵ and
                             |p| ≤ 2 · 4095² < 2²⁶ at their bounds; Σx of a full mask ≈ 3.4e10

CPU time of the golden model on these inputs, single-threaded, measured once on the development host (the
budget of a GPU test is a few seconds, nearly all of it spent here):
  golden_measure            full 4096²: 0.89 s   a sparse mask at 4096²: 0.43 s
                            at 4096 × 600: full 0.06 s, checkerboard 0.05 s, noise_0.593 0.21 s
  golden_measure_diameters  full 4096²: 0.87 s   a sparse mask at 4096²: 0.23–0.32 s   at 4096 × 600: ≤ 0.08 s
  golden_run (every stage, renders, JPEGs)  1100 × 1040: 0.57 s   4096 × 100: 0.20 s
  diameter_masks.brute_force on the row extremes  frame (8190 points): 2.4 s   a diagonal (4096): 0.8–1.2 s
  NumPy  full 4096²: 0.02 s   raw_of(4096, 4096): 0.06 s   spiral 4096 × 100: 0.12 s, 1100 × 1040: 0.43 s
No call reaches 5 s, so square_limit keeps its K7 and K9 cases (whose goldens are linear in the pixels
plus quadratic in at most 8192 candidates); the K1 / K2 lists never held it."""
import functools

import numpy as np

import diameter_masks as dm
import measure_masks as mm

LIMIT = 4096  # gpu_types.h kMaxSliceDim
WRAP = 1024   # threads of a K2 / K7 / K9 workgroup: a strided loop over rows or columns wraps above it

SHAPES = {"rows_wrap": (1030, 70), "cols_wrap": (70, 1030), "both_wrap": (1100, 1040), "tall_limit": (4096, 100),
          "wide_limit": (100, 4096), "sum64": (4096, 600), "square_limit": (4096, 4096)}

# ---- K2 -------------------------------------------------------------------------------------------
K2_SHAPES = ("rows_wrap", "cols_wrap", "both_wrap", "tall_limit", "wide_limit")
K2_BANDS = ("serpentine", "serpentine_v", "spiral", "comb", "noise_0.593")
ISLAND = 10  # the island's centre lies this far inside the bottom-right corner


def lines_of(h, w):
    """(x of the vertical line or None, y of the horizontal line or None): a one-pixel line along every
    side longer than WRAP, through the centre, where reference_seeds puts its first seed."""
    return (w // 2 if h > WRAP else None, h // 2 if w > WRAP else None)


@functools.lru_cache(maxsize=None)
def k2_band(name, h, w):
    """The named measure_masks mask with a one-pixel line ORed in along every side longer than WRAP (so
    a region seeded anywhere on it crosses row / column 1024 and reaches the far edge), and one island:
    a band pixel in a cleared 5 × 5 window near the bottom-right corner, which no seed reaches, so the
    region is never the whole band."""
    b = mm.build(name, h, w).copy()
    xl, yl = lines_of(h, w)
    cy, cx = h - ISLAND, w - ISLAND
    b[cy - 2:cy + 3, cx - 2:cx + 3] = False
    b[cy, cx] = True
    if xl is not None:
        b[:, xl] = True
    if yl is not None:
        b[yl, :] = True
    b.setflags(write=False)
    return b


def k2_seeds(reference_seeds, h, w):
    """(x, y, 0) seeds: the pipeline's (`reference_seeds` = native.reference_seeds(w, h)) plus one at the
    far end of every line of lines_of."""
    xl, yl = lines_of(h, w)
    seeds = [(x, y, 0) for (x, y) in reference_seeds]
    if xl is not None:
        seeds.append((xl, h - 1, 0))
    if yl is not None:
        seeds.append((w - 1, yl, 0))
    return seeds


def label_region(band, seeds, conn):
    """Seeded region growing by scipy.ndimage.label: the union of the components of `band` (at `conn`
    4 | 8) that hold an in-image, in-band seed. Shares nothing with the golden model's flood fill."""
    from scipy import ndimage
    h, w = band.shape
    lab, _ = ndimage.label(band, structure=ndimage.generate_binary_structure(2, 2 if conn == 8 else 1))
    hit = {int(lab[y, x]) for (x, y, *_r) in seeds if 0 <= x < w and 0 <= y < h and band[y, x]}
    return np.isin(lab, sorted(hit)) & band if hit else np.zeros_like(band)


MORPH_WIDE = (63, 9, 5)  # dilation, erosion, border radius of the wide-shift case at cols_wrap


@functools.lru_cache(maxsize=None)
def morph_band(h, w):
    """The band of the wide-shift morphology case (made for cols_wrap): an 11-row bar from column 100 to
    the right edge with one-pixel holes in the words on both sides of three word boundaries, and a block of its own in the
    top-left corner that no seed reaches. A 63-wide dilation of the bar (shifts of up to 31 bits across
    the 17 words) leaves the columns left of 69 clear; a 9-wide erosion leaves three rows of it, wiped
    around the holes; the border of radius 5 keeps all but one row."""
    assert h >= 60 and w >= 700
    b = np.zeros((h, w), bool)
    y0 = h // 2 - 5
    b[y0:y0 + 11, 100:] = True
    for x in (191, 192, 575, 640, 1023, 1024):  # in the top row: the erosion wipes the first of its three rows around them
        b[y0, x] = False
    b[y0 + 5, 700] = False                      # in the middle row: wipes all three
    b[2:7, 10:31] = True
    b.setflags(write=False)
    return b


def morph_seeds(reference_seeds, h, w):
    return [(x, y, 0) for (x, y) in reference_seeds] + [(w - 1, h // 2 - 2, 0)]


# ---- K7 / K9 ----------------------------------------------------------------------------------------
MEASURE_SHAPES = ("rows_wrap", "cols_wrap", "tall_limit", "wide_limit")  # every named mask, one launch
SUM64_MASKS = ("full", "checkerboard", "serpentine", "noise_0.593")
SPARSE = ("diag_main", "diag_anti", "frame", "blobs_diag", "bars_far")
# Connectivities at which a sparse mask is ONE component (a diagonal's pixels touch at corners only).
SPARSE_CONN = {"diag_main": (8,), "diag_anti": (8,), "frame": (4, 8), "blobs_diag": (8,), "bars_far": (4, 8)}
_F = LIMIT - 1
# The analytic record of every sparse mask at square_limit: major_px2, major [xa, ya, xb, yb],
# perp_extent, perp [xc, yc, xd, yd]. a < b in (y, x) order; of equal pairs the first a, then the first
# b; of equal projections p = −dy·x + dx·y (dx = xb − xa, dy = yb − ya) the first pixel in (y, x) order.
#   diag_main: every p is 0: both perp ends are the first pixel.
#   diag_anti: a = (y 0, x 4095), b = (y 4095, x 0); p = −4095·(x + y) = −4095² everywhere.
#   frame: the two diagonals of the square tie; a = (0, 0) comes first. p = 4095·(y − x): least at the
#       top-right corner, greatest at the bottom-left one: the extent is 2 · 4095² too.
#   blobs_diag: 3 × 3 blobs in the corners: p = 4095·(y − x) is least at (y 0, x 2), greatest at (y 2, x 0).
#   bars_far: row 4095 and column 4095. a = (y 0, x 4095), b = (y 4095, x 0); p = −4095·(x + y) is least
#       at the corner (4095, 4095), where |p| = 2 · 4095² is the largest the engine can meet, and
#       greatest (−4095²) at both bar ends, of which (y 0, x 4095) comes first.
SPARSE_EXPECT = {
    "diag_main": (2 * _F * _F, [0, 0, _F, _F], 0, [0, 0, 0, 0]),
    "diag_anti": (2 * _F * _F, [_F, 0, 0, _F], 0, [_F, 0, _F, 0]),
    "frame": (2 * _F * _F, [0, 0, _F, _F], 2 * _F * _F, [_F, 0, 0, _F]),
    "blobs_diag": (2 * _F * _F, [0, 0, _F, _F], 4 * _F, [2, 0, 0, 2]),
    "bars_far": (2 * _F * _F, [_F, 0, 0, _F], _F * _F, [_F, _F, _F, 0]),
}


@functools.lru_cache(maxsize=None)
def sparse(name, side=LIMIT):
    """The named sparse mask at side × side (cached, read-only)."""
    m = np.zeros((side, side), bool)
    i = np.arange(side)
    if name == "diag_main":
        m[i, i] = True
    elif name == "diag_anti":
        m[i, side - 1 - i] = True
    elif name == "frame":
        m[0, :] = m[side - 1, :] = True
        m[:, 0] = m[:, side - 1] = True
    elif name == "blobs_diag":
        m[i, i] = True
        m[:3, :3] = True
        m[side - 3:, side - 3:] = True
    elif name == "bars_far":
        m[side - 1, :] = True
        m[:, side - 1] = True
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


def measure_mask(name, h, w):
    """A mask by name at h × w: the sparse ones (square only), else diameter_masks' (which hold measure_masks')."""
    if name in SPARSE:
        assert h == w
        return sparse(name, h)
    return dm.build(name, h, w)


def row_extremes(lesion):
    """The leftmost and the rightmost pixel of every row of `lesion` (bool [h, w]) as a mask: K9's candidates."""
    out = np.zeros_like(lesion)
    rows = np.flatnonzero(lesion.any(axis=1))
    out[rows, lesion[rows].argmax(axis=1)] = True
    out[rows, lesion.shape[1] - 1 - lesion[rows, ::-1].argmax(axis=1)] = True
    return out


def lesion_of(mask, conn):
    """The largest component of `mask` at `conn` (the first one in raster order of equal ones) by scipy."""
    from scipy import ndimage
    lab, ncomp = ndimage.label(mask, structure=ndimage.generate_binary_structure(2, 2 if conn == 8 else 1))
    if ncomp == 0:
        return np.zeros_like(mask)
    return lab == int(np.argmax(np.bincount(lab.ravel())[1:])) + 1


@functools.lru_cache(maxsize=None)
def brute_force_on_extremes(name, h, w, conn):
    """diameter_masks.brute_force restricted to the row extremes of the lesion (the brute force over all
    pixels is O(n²)): (major_px2, major, perp_extent, perp), or None for an empty mask."""
    les = lesion_of(measure_mask(name, h, w), conn)
    if not les.any():
        return None
    return dm.brute_force(row_extremes(les))


def full_closed_form(h, w, raw):
    """The K7 record of the full h × w mask in closed form (raw_sum from NumPy in int64)."""
    v = raw.astype(np.int64)
    return {"area_px": h * w, "bbox": [0, 0, w - 1, h - 1], "sum_x": h * (w * (w - 1) // 2), "sum_y": w * (h * (h - 1) // 2),
            "perimeter_edges": 2 * (h + w), "components": 1, "largest_px": h * w, "holes": 0,
            "raw_sum": int(v.sum()), "raw_min": int(v.min()), "raw_max": int(v.max())}


# ---- K1a / K1b --------------------------------------------------------------------------------------
K1_SHAPES = ("cols_wrap", "rows_wrap", "wide_limit", "tall_limit")


def edge_ramp(h, w):
    """12-bit values that differ from pixel to pixel in the last tile column and row: 7·x + 13·y mod 4093
    (a prime), so a median or a blur that reads a neighbouring tile's column or row gives another value."""
    y, x = np.mgrid[0:h, 0:w]
    return ((7 * x + 13 * y) % 4093).astype(np.uint16)


# ---- render / engine --------------------------------------------------------------------------------
RENDER_CASES = (("tall_limit", 512, 512), ("wide_limit", 512, 512), ("both_wrap", 512, 512), ("both_wrap", 384, 512))  # out_w, out_h
ENGINE_SHAPES = ("both_wrap", "tall_limit", "wide_limit")
# The engine refuses slices with a side below PipelineParams::min_dim (100 by default) as too small, and
# the command-line tools have no flag for it: where a file goes through them, rows_wrap is widened to
# that minimum (still two rows per K2 thread, 17 words per transposed row). An Engine of the tests'
# own takes min_dim = MIXED_MIN_DIM and the 70-wide shapes as they are.
ROWS_WRAP_FILE = (1030, 100)
MIXED_MIN_DIM = 64
BRIDGE_VALUE = 1500  # normalises to 0.8, inside the default band [0.74, 0.91]
BRIDGE_HALF = 12     # half-width: the 7-wide median and the 9-wide sharpen leave the bridge's core in the band


def bridged(phantom, h, w):
    """`phantom` (uint16 [h, w], native.phantom_slice) with a band-valued bridge 2·BRIDGE_HALF wide along
    every side longer than WRAP, through the centre seed: the grown region spans the wrap boundary. A
    24 × 24 patch of the same value in the top-left corner is band that no seed reaches."""
    a = np.array(phantom, dtype=np.uint16)
    xl, yl = lines_of(h, w)
    a[4:28, 4:28] = BRIDGE_VALUE
    if xl is not None:
        a[:, xl - BRIDGE_HALF:xl + BRIDGE_HALF] = BRIDGE_VALUE
    if yl is not None:
        a[yl - BRIDGE_HALF:yl + BRIDGE_HALF, :] = BRIDGE_VALUE
    return a


def spans_wrap(region, h, w):
    """The region holds pixels on both sides of row / column WRAP of every side longer than WRAP."""
    ys, xs = np.nonzero(region)
    ok = len(ys) > 0
    if h > WRAP:
        ok = ok and ys.min() < WRAP <= ys.max()
    if w > WRAP:
        ok = ok and xs.min() < WRAP <= xs.max()
    return bool(ok)
