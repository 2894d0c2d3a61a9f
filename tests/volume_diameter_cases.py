"""Inputs of the per-lesion diameter tests (test_volume_diameters.py on the CPU,
test_gpu_volume_diameters.py on the GPU; not a conftest). Builds on volume_lesion_cases and
volume_measure_cases and adds the shapes at which the row extremes, their attribution to a lesion, the
tie rules, the physical (not voxel) maximisation and the tile skipping can go wrong. Everything is NumPy
on the CPU; masks are uint8 [d, h, w]."""
import os
import re

import numpy as np

import volume_lesion_cases as vlc
import volume_measure_cases as vmc

CONNS = (6, 26)
SPACINGS = ((1000, 1000, 1000), (500, 500, 5000), (977, 1020, 3300))
INT_KEYS = ("major_um2", "major", "axial_z", "axial_um2", "axial", "axial_perp_extent", "axial_perp")

# The worked example of nm03/measure.h: the box x 0…9, y 0…3, z 0…2 at 1 mm isotropic.
HAND = {"major_um2": 94_000_000, "major": [0, 0, 0, 9, 3, 2], "axial_z": 0, "axial_um2": 90_000_000,
        "axial": [0, 0, 9, 3], "axial_perp_extent": 54, "axial_perp": [9, 0, 0, 3]}


def hand_box():
    m = np.zeros((4, 6, 12), np.uint8)
    m[0:3, 0:4, 0:10] = 1
    return m


def one_voxel():
    m = np.zeros((3, 4, 70), np.uint8)
    m[1, 2, 65] = 1
    return m


def needle():
    """One voxel per plane: axial_um2 = 0 in the first plane."""
    m = np.zeros((9, 4, 5), np.uint8)
    m[2:, 2, 3] = 1
    return m


def specks():
    """One-voxel lesions on a lattice of stride 3 (no contact at 26 either): more than 64 of them."""
    rng = np.random.default_rng(5)
    m = np.zeros((7, 13, 70), np.uint8)
    m[::3, ::3, ::3] = rng.random(m[::3, ::3, ::3].shape) < 0.5
    return m


def combs():
    """Two combs whose teeth interleave: rows 2 … 8 hold teeth of both, A B A B …, across the word edge."""
    m = np.zeros((3, 11, 72), np.uint8)
    m[0:2, 0, 0:70] = 1
    m[0:2, 10, 2:72] = 1
    for x in range(0, 70, 8):
        m[0:2, 0:9, x] = 1        # A: down from the upper spine
        m[0:2, 2:11, x + 4] = 1   # B: up from the lower spine
    return m


def cube():
    m = np.zeros((14, 14, 14), np.uint8)
    m[1:13, 1:13, 1:13] = 1
    return m


def ball(r=9):
    n = 2 * r + 3
    z, y, x = np.ogrid[:n, :n, :n]
    c = r + 1
    return ((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2 <= r * r).astype(np.uint8)


def l_shape():
    """A bar along x (x 0 … 19) with a bar along z (z 0 … 5) standing on x = 12: in voxel units the bar's
    ends are the farthest pair, at uz = 5000 against ux = 500 the pair (0, 0, 0) – (12, 0, 5) is."""
    m = np.zeros((7, 3, 22), np.uint8)
    m[0, 0, 0:20] = 1
    m[0:6, 0, 12] = 1
    return m


def ellipsoid():
    """Radii (14, 18, 30) in x, y, z, centred on the word edge x = 64: more than 1024 row extremes, so
    several tiles and several workgroups, and tile pairs the bound really skips."""
    z, y, x = np.ogrid[:63, :39, :80]
    return (((x - 64) / 14.0) ** 2 + ((y - 19) / 18.0) ** 2 + ((z - 31) / 30.0) ** 2 <= 1.0).astype(np.uint8)


# The largest spacings the ellipsoid's frame (80 × 39 × 63) admits: every axis extent just below 2^31 um, so
# a squared distance across the frame approaches 3 · 2^62 and is ordered right only as an unsigned 64-bit number.
ELLIPSOID_MAX_UM = ((2 ** 31 - 1) // 79, (2 ** 31 - 1) // 38, (2 ** 31 - 1) // 62)


def split_section():
    """Two pillars joined by a bridge on top: the section of plane 0 … 2 is two separate blobs, and the
    axial pair spans both."""
    m = np.zeros((5, 6, 70), np.uint8)
    m[0:4, 1:3, 60:63] = 1
    m[0:4, 3:5, 66:69] = 1
    m[3, 1:5, 60:69] = 1
    return m


# (id, mask builder, N)
CASES = [
    ("hand_box", hand_box, 1),
    ("one_voxel", one_voxel, 2),
    ("needle", needle, 1),
    ("empty", lambda: vmc.empty((3, 5, 70)), 3),
    ("full", lambda: vmc.full((4, 5, 66)), 3),
    ("equal_boxes", vlc.equal_boxes, 3),
    ("equal_boxes_swapped", vlc.equal_boxes_swapped, 3),
    ("word_straddle-64", lambda: vlc.word_straddle(64), 3),
    ("word_straddle-65", lambda: vlc.word_straddle(65), 3),
    ("word_straddle-130", lambda: vlc.word_straddle(130), 3),
    ("corner_chain", vlc.corner_chain, 8),
    ("specks", specks, 64),
    ("combs", combs, 2),
    ("cube", cube, 1),
    ("ball", ball, 1),
    ("l_shape", l_shape, 1),
    ("ellipsoid", ellipsoid, 2),
    ("split_section", split_section, 1),
]


def cpu_cases():
    return CASES


def gpu_cases():
    """cpu_cases() plus the GPU_EXTRA_SHAPE variants (more words per plane than a workgroup has threads)."""
    s = vmc.GPU_EXTRA_SHAPE
    sid = vmc.shape_id(s)
    return CASES + [(f"word_edges-{sid}", lambda: vmc.word_edges(s), 8), (f"corners-{sid}", lambda: vmc.corners(s), 8),
                    (f"noise0.1-{sid}", lambda: vmc.noise(s, 0.1), 16), (f"noise0.31-{sid}", lambda: vmc.noise(s, 0.31), 4)]


def pair_holds(rec, um):
    """The record's own consistency: the squared lengths are those of the voxels it names, a does not
    follow b, and the extent is that of c and d on the axial pair's normal."""
    xa, ya, za, xb, yb, zb = rec["major"]
    ok = rec["major_um2"] == ((xb - xa) * um[0]) ** 2 + ((yb - ya) * um[1]) ** 2 + ((zb - za) * um[2]) ** 2
    ok &= (za, ya, xa) <= (zb, yb, xb)
    xa, ya, xb, yb = rec["axial"]
    ok &= rec["axial_um2"] == ((xb - xa) * um[0]) ** 2 + ((yb - ya) * um[1]) ** 2
    ok &= (ya, xa) <= (yb, xb)
    dx, dy = xb - xa, yb - ya
    xc, yc, xd, yd = rec["axial_perp"]
    ok &= rec["axial_perp_extent"] == (-dy * xd + dx * yd) - (-dy * xc + dx * yc)
    return bool(ok)


# The new keys as the sidecar writer puts them: one before lesions_max, one run per lesion object after `mean`.
NEW_KEYS = re.compile(r',"diameters_spacing_um":\[[0-9,]*\]|,"major_um2":[^}]*')


def strip_new_keys(text):
    """A flagged sidecar's text without the diameter keys: the unflagged text, byte for byte."""
    return NEW_KEYS.sub("", text)


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out
