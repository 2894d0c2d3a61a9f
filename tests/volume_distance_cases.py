"""Shared cases of the distance-map tests (nm03/volume_distance.h, K16): masks as uint8 [D, H, W], spacings in
integer micrometres (ux, uy, uz), and the caps each case is run at (None = no cap). Every comparison made with
them is == on integers, bits and text."""
import numpy as np

NO_DISTANCE = 2 ** 63 - 1
POLARITIES = ("foreground", "background")
ISO = (1000, 1000, 1000)
COPRIME = (391, 703, 6500)
NEAR_EXTENT_UM = (300_000_000, 600_000_000, 600_000_000)
# the thickness of the INVERSE of near_extent's mask: the far corner (4, 2, 2), whose only background voxel is the
# origin; 4.32e18 fills the high half of the 64-bit shuffles of the reduction
NEAR_EXTENT_INVERSE_THICKNESS = {"inscribed_um2": 4_320_000_000_000_000_000, "inscribed_at": [4, 2, 2], "found": True}


def _noise(shape, density, seed):
    rng = np.random.RandomState(seed)
    return (rng.random_sample(shape) < density).astype(np.uint8)


def _points(shape, pts):
    m = np.zeros(shape, np.uint8)
    for x, y, z in pts:
        m[z, y, x] = 1
    return m


def _case(name, mask, um, caps=None):
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    mask.setflags(write=False)
    ux = int(um[0])
    # cap at 0; exactly on (ux)², attained wherever the nearest S voxel is the x neighbour; 1.5·ux, between two
    # attained distances of every case here
    return {"name": name, "mask": mask, "um": tuple(int(v) for v in um), "caps": caps or (None, 0, ux, ux + ux // 2)}


def all_cases():
    small = (4, 6, 70)
    corners = _points(small, [(x, y, z) for x in (0, 69) for y in (0, 5) for z in (0, 3)])
    two = np.zeros((3, 5, 12), np.uint8)  # two 3×3×3 cubes: their centres tie for the thickness
    two[0:3, 1:4, 1:4] = 1
    two[0:3, 1:4, 7:10] = 1
    zz, yy, xx = np.indices((5, 7, 66))
    checker = ((xx + yy + zz) & 1).astype(np.uint8)
    plane = np.zeros((6, 8, 66), np.uint8)
    plane[3] = 1
    long_col = np.zeros((1, 300, 2), np.uint8)
    long_col[0, 0, 1] = 1
    long_line = np.zeros((300, 1, 2), np.uint8)
    long_line[299, 0, 1] = 1
    return [
        _case("worked_example", _points((5, 21, 21), [(10, 10, 2)]), (500, 500, 5000), (None, 0, 500, 5000, 5001, 700)),
        _case("width_70", _noise((3, 9, 70), 0.3, 1), ISO),
        _case("many_workgroups", _noise((12, 40, 130), 0.05, 2), COPRIME),
        _case("line_x", _points((1, 1, 200), [(3, 0, 0), (64, 0, 0), (190, 0, 0)]), (700, 1000, 1000)),
        _case("line_y", _points((1, 37, 1), [(0, 5, 0), (0, 30, 0)]), (1000, 300, 1000)),
        _case("line_z", _points((9, 1, 1), [(0, 0, 7)]), (1000, 1000, 2500)),
        _case("long_column", long_col, (1000, 800, 1000)),
        _case("long_column_noise", _noise((1, 300, 2), 0.02, 3), (1000, 800, 1000)),
        _case("empty", np.zeros(small, np.uint8), ISO),
        _case("full", np.ones(small, np.uint8), ISO),
        _case("corners", corners, (900, 1100, 2000)),
        _case("two_cubes_tie", two, ISO),
        _case("checkerboard", checker, (600, 700, 800)),
        _case("one_plane", plane, (1000, 1000, 3000)),
        _case("noise_50", _noise((5, 11, 67), 0.5, 4), (500, 750, 5000)),
        _case("noise_0p2", _noise((12, 40, 130), 0.002, 5), ISO),
        _case("corner_voxel", _points((12, 40, 130), [(0, 0, 0)]), COPRIME),
        _case("anisotropic_nearest", _points((3, 3, 9), [(4, 1, 2), (8, 1, 1)]), (1000, 1000, 5000)),
        _case("word_edges", _points((2, 3, 129), [(63, 0, 0), (64, 1, 0), (128, 2, 1), (0, 2, 0)]), (1000, 1200, 900)),
        # more than 64 words per row: the rows pass looks at the row's words 64 at a time, and here the nearest set
        # word lies in the same group of 64 (row 0), in the group before (row 1) and in the group after (row 2)
        _case("row_of_66_words", _points((1, 3, 4200), [(5, 0, 0), (4100, 0, 0), (5, 1, 0), (4190, 2, 0)]), (300, 90000, 1000)),
        # just below the extent limit: every axis spans 1.2e9 um < 2^31, the far corner lies at 4.32e18 < 2^62. The cap
        # 2e9 drops that corner alone; 2^31 - 1 is the last cap that is squared, 2^31 the first that becomes 2^62
        _case("near_extent", _points((3, 3, 5), [(0, 0, 0)]), NEAR_EXTENT_UM, (None, 0, 300_000_000, 2_000_000_000, 2 ** 31 - 1, 2 ** 31)),
        # the planes pass searches 299 steps along z: the maximum, (299 * 800)^2 + 1000^2 = 57 217 640 000, at (0, 0, 0)
        _case("long_plane_line", long_line, (1000, 1000, 800)),
    ]


def ids(cases):
    return [c["name"] for c in cases]


def case(name):
    return next(c for c in all_cases() if c["name"] == name)


def voxels(c):
    return int(np.prod(c["mask"].shape))


def ball(k):
    """The digital ball of radius k index steps in a frame with one background voxel of margin on every side."""
    n = 2 * k + 3
    zz, yy, xx = np.indices((n, n, n)) - (k + 1)
    return (xx * xx + yy * yy + zz * zz <= k * k).astype(np.uint8)


def thickness_equal(a, b):
    return all(a[k] == b[k] for k in ("inscribed_um2", "inscribed_at", "found", "inscribed_radius_mm", "thickness_mm"))
