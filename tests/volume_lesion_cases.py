"""Inputs of the per-lesion volume measurement tests (test_volume_lesions.py on the CPU,
test_gpu_volume_lesions.py on the GPU; not a conftest). Builds on volume_measure_cases and adds the
shapes at which the SELECTION of the N largest components and the ATTRIBUTION of voxels, faces and
samples to a lesion can go wrong. Everything is NumPy on the CPU; masks are uint8 [d, h, w]."""
import numpy as np

import volume_measure_cases as vmc

CONNS = (6, 26)
LESION_COUNTS = (1, 3, 64)
INT_KEYS = ("voxels", "first", "bbox", "sum_x", "sum_y", "sum_z", "faces_x", "faces_y", "faces_z", "raw_sum", "raw_min",
            "raw_max")
DERIVED_KEYS = ("volume_mm3", "volume_ml", "surface_mm2", "equivalent_diameter_mm", "centroid_x", "centroid_y",
                "centroid_z", "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean")


def _boxes(shape, *boxes):
    m = np.zeros(shape, np.uint8)
    for z0, z1, y0, y1, x0, x1 in boxes:
        m[z0:z1, y0:y1, x0:x1] = 1
    return m


def equal_boxes():
    """Two 2 × 3 × 4 boxes of equal size: the one first in raster order (the upper plane) comes first."""
    return _boxes((8, 10, 20), (1, 3, 5, 8, 10, 14), (5, 7, 1, 4, 2, 6))


def equal_boxes_swapped():
    """The same two boxes with their z ranges exchanged: the other one is now first."""
    return _boxes((8, 10, 20), (5, 7, 5, 8, 10, 14), (1, 3, 1, 4, 2, 6))


def word_straddle(w):
    """A box across x = 63 / 64 (as far as the width reaches) and a larger one whose last voxels lie in the
    last column of a width-w volume: w = 65 (the last column is bit 0 of a second word), 64 (bit 63 of
    the only word) and 130 (both boxes cross a word edge, the second one ends the third word)."""
    return _boxes((6, 9, w), (1, 3, 1, 4, 60, min(68, w)), (3, 6, 5, 9, w - 4, w))


def frame_toucher():
    """A cross whose arms reach all six frame faces (its end faces lie against the frame), and a speck."""
    m = np.zeros((7, 9, 70), np.uint8)
    m[3, 4, :] = 1
    m[3, :, 33] = 1
    m[:, 4, 33] = 1
    m[0, 0, 0] = 1
    return m


def corner_chain():
    """Voxels that meet only at corners and edges: one lesion at 26-connectivity, several at 6."""
    m = np.zeros((4, 4, 66), np.uint8)
    m[0, 0, 62] = m[1, 1, 63] = m[2, 2, 64] = m[3, 3, 65] = 1  # corners, across the word edge
    m[0, 3, 10] = m[0, 2, 11] = 1                              # an edge contact in one plane
    return m


def speck_noise():
    """Hundreds of one-voxel components: massive ties, decided by the first voxel alone."""
    return vmc.noise(vmc.NOISE_SHAPE, 0.1)


EXTRA_CASES = [
    ("equal_boxes", equal_boxes),
    ("equal_boxes_swapped", equal_boxes_swapped),
    ("word_straddle-65", lambda: word_straddle(65)),
    ("word_straddle-64", lambda: word_straddle(64)),
    ("word_straddle-130", lambda: word_straddle(130)),
    ("frame_toucher", frame_toucher),
    ("corner_chain", corner_chain),
    ("speck_noise", speck_noise),
    ("empty", lambda: vmc.empty((3, 5, 70))),
    ("full", lambda: vmc.full((3, 5, 70))),
]


def cpu_cases():
    """(id, mask builder): every case of volume_measure_cases, then the lesion shapes."""
    return vmc.all_cases() + EXTRA_CASES


def gpu_cases():
    """cpu_cases() plus the GPU_EXTRA_SHAPE variants (more words per plane than a workgroup has threads)."""
    s = vmc.GPU_EXTRA_SHAPE
    sid = vmc.shape_id(s)
    return cpu_cases() + [(f"word_edges-{sid}", lambda: vmc.word_edges(s)), (f"corners-{sid}", lambda: vmc.corners(s)),
                          (f"noise0.1-{sid}", lambda: vmc.noise(s, 0.1)), (f"noise0.31-{sid}", lambda: vmc.noise(s, 0.31))]


def inputs(mask, seed=0):
    """(region, raw) for a mask: a region of another voxel count, samples of every bit pattern."""
    return vmc.region_for(mask), vmc.raw_for(mask.shape, seed)


def order_holds(lesions):
    """voxels descending; among equals the first voxel ascending in raster (z, y, x) order."""
    keys = [(-l["voxels"], l["first"][2], l["first"][1], l["first"][0]) for l in lesions]
    return keys == sorted(keys) and len(set(keys)) == len(keys)
