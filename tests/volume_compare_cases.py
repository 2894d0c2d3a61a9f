"""Shared cases of the comparison tests (nm03/volume_compare.h, K17): pairs of masks as uint8 [D, H, W], a spacing in
integer micrometres (ux, uy, uz) and, where a case claims something about itself, that claim — checked by
test_volume_compare_cases.py, so that a later edit of a mask cannot empty a test. Every comparison made with them
is == on integers and text."""
import numpy as np

ISO = (1000, 1000, 1000)
ANISO = (500, 500, 5000)
COPRIME = (391, 703, 6500)

# The kernels' constants (src/kernels/k17_volume_compare.hip): 256 words per block, at most 1024 blocks per
# sampling launch. A second trip of a workgroup's strided loop needs more than MAX_BLOCKS · 256 words; "size"
# (130 × 40 × 24: 3 · 40 · 24 = 2880 words, 12 blocks) runs at max_blocks = 5, so a workgroup takes 3 trips (the
# last one partial: blocks 10 and 11 only) and every launch but the one-workgroup ones has several workgroups.
WORDS_PER_BLOCK = 256
MAX_BLOCKS = 1024
SIZE_MAX_BLOCKS = 5

DIGIT_SHIFT = (21, 10, 0)  # 11 + 11 + 10 bits
DIGIT_BINS = (2048, 2048, 1024)


def _noise(shape, density, seed):
    return (np.random.RandomState(seed).random_sample(shape) < density).astype(np.uint8)


def _points(shape, pts):
    m = np.zeros(shape, np.uint8)
    for x, y, z in pts:
        m[z, y, x] = 1
    return m


def _box(shape, xs, ys, zs):
    m = np.zeros(shape, np.uint8)
    m[zs[0]:zs[1] + 1, ys[0]:ys[1] + 1, xs[0]:xs[1] + 1] = 1
    return m


def _ball(shape, c, r):
    zz, yy, xx = np.indices(shape)
    return ((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2 <= r * r).astype(np.uint8)


def _case(name, a, b, um=ISO, **claims):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    assert a.shape == b.shape and a.ndim == 3, name
    a.setflags(write=False)
    b.setflags(write=False)
    c = {"name": name, "a": a, "b": b, "um": tuple(int(v) for v in um), "max_blocks": None}
    c.update(claims)
    return c


# The three worked examples of nm03/volume_compare.h, every integer of the record.
WORKED = {
    "worked_boxes": {"a_vox": 120, "b_vox": 289, "tp_vox": 48, "fp_vox": 72, "fn_vox": 241, "surface_a": 104, "surface_b": 209,
                     "n_ab": 104, "max_um2_ab": 11_250_000, "sum_um_ab": 164_741, "p95_um_ab": 2692, "found_ab": True,
                     "n_ba": 209, "max_um2_ba": 70_000_000, "sum_um_ba": 716_543, "p95_um_ba": 5916, "found_ba": True},
    "worked_nested": {"a_vox": 27, "b_vox": 729, "tp_vox": 27, "fp_vox": 0, "fn_vox": 702, "surface_a": 26, "surface_b": 386,
                      "n_ab": 26, "max_um2_ab": 9_000_000, "sum_um_ab": 78_000, "p95_um_ab": 3000, "found_ab": True,
                      "n_ba": 386, "max_um2_ba": 27_000_000, "sum_um_ba": 1_418_760, "p95_um_ba": 4690, "found_ba": True},
    "worked_2_24": {"a_vox": 1, "b_vox": 1, "tp_vox": 0, "fp_vox": 1, "fn_vox": 1, "surface_a": 1, "surface_b": 1,
                    "n_ab": 1, "max_um2_ab": 784_000_000_000_000, "worst_ab": [0, 0, 0], "sum_um_ab": 28_000_000,
                    "p95_um_ab": 28_000_000, "found_ab": True,
                    "n_ba": 1, "max_um2_ba": 784_000_000_000_000, "worst_ba": [7, 0, 0], "sum_um_ba": 28_000_000,
                    "p95_um_ba": 28_000_000, "found_ba": True},
}
WORKED_ISQRT = {11_250_000: 3354, 70_000_000: 8366, 784_000_000_000_000: 28_000_000}


def _width_case(w):
    # A: a slab that runs through every word edge of the row (x 0 … w − 1 in rows 1 and 2 of plane 1) plus single voxels
    # on both sides of each edge; B: noise, so that the carries of both masks are exercised at every x
    shape = (3, 4, w)
    a = np.zeros(shape, np.uint8)
    a[1, 1:3, :] = 1
    for x in (0, 62, 63, 64, 65, 127, 128, 129):
        if x < w:
            a[0, 0, x] = 1
            a[2, 3, x] = 1
    return _case(f"width_{w}", a, _noise(shape, 0.7, 100 + w), ISO, width=w)


def all_cases():
    cases = [_width_case(w) for w in (1, 63, 64, 65, 130)]
    small = (4, 6, 70)
    frame = np.zeros((5, 6, 66), np.uint8)  # every voxel on a face of the frame
    frame[0] = frame[-1] = 1
    frame[:, 0] = frame[:, -1] = 1
    frame[:, :, 0] = frame[:, :, -1] = 1
    noise_a = _noise((5, 11, 67), 0.5, 11)
    size_shape = (24, 40, 130)
    size_a = _ball(size_shape, (60, 20, 12), 9) | _noise(size_shape, 0.002, 21)
    size_b = _ball(size_shape, (66, 18, 11), 10) | _noise(size_shape, 0.002, 22)
    cases += [
        _case("thin_d1", _noise((1, 9, 70), 0.4, 1), _noise((1, 9, 70), 0.4, 2), COPRIME),
        _case("thin_h1", _noise((5, 1, 70), 0.4, 3), _noise((5, 1, 70), 0.4, 4), COPRIME),
        _case("frame_faces", frame, _box((5, 6, 66), (1, 64), (1, 4), (1, 3)), ISO),
        # the full 3 × 3 × 3 frame has 26 surface voxels: only the centre has six neighbours
        _case("full_3x3x3", np.ones((3, 3, 3), np.uint8), _points((3, 3, 3), [(1, 1, 1)]), ISO, surface_a=26, surface_b=1),
        # a 5³ cube inside a 7³ frame has 98
        _case("cube_5_in_7", _box((7, 7, 7), (1, 5), (1, 5), (1, 5)), np.ones((7, 7, 7), np.uint8), ISO, surface_a=98),
        _case("equal", _noise(small, 0.3, 5), _noise(small, 0.3, 5), COPRIME, equal=True),
        _case("disjoint", _box(small, (0, 20), (0, 2), (0, 1)), _box(small, (40, 69), (3, 5), (2, 3)), ISO, tp_vox=0),
        _case("a_empty", np.zeros(small, np.uint8), _noise(small, 0.3, 6), ISO, found=False),
        _case("b_empty", _noise(small, 0.3, 7), np.zeros(small, np.uint8), ISO, found=False),
        _case("both_empty", np.zeros(small, np.uint8), np.zeros(small, np.uint8), ISO, found=False),
        _case("single_voxels", _points(small, [(3, 1, 0)]), _points(small, [(66, 4, 3)]), COPRIME),
        _case("worked_boxes", _box((5, 8, 16), (0, 9), (0, 3), (0, 2)),
              _box((5, 8, 16), (2, 13), (1, 6), (1, 4)) | _points((5, 8, 16), [(15, 6, 4)]), (1000, 1000, 2500)),
        _case("worked_nested", _box((11, 11, 11), (4, 6), (4, 6), (4, 6)), _box((11, 11, 11), (1, 9), (1, 9), (1, 9)), ISO),
        _case("worked_2_24", _points((1, 1, 8), [(0, 0, 0)]), _points((1, 1, 8), [(7, 0, 0)]), (4_000_000, 1000, 1000)),
        _case("anisotropic", _ball((5, 21, 21), (8, 10, 2), 5), _ball((5, 21, 21), (12, 11, 2), 6), ANISO),
        # two voxels of A at one distance from B's only voxel, in rows 0 and 4 / in planes 0 and 2: the first in raster
        # order is the worst
        _case("tie_rows", _points((3, 5, 11), [(5, 0, 1), (5, 4, 1)]), _points((3, 5, 11), [(5, 2, 1)]), ISO, worst_ab=[5, 0, 1]),
        _case("tie_planes", _points((3, 5, 11), [(5, 2, 0), (5, 2, 2)]), _points((3, 5, 11), [(5, 2, 1)]), ISO, worst_ab=[5, 2, 0]),
        # one plane: every voxel is a surface voxel. 95 · n is a multiple of 100 for n = 20 (k = 19) and n = 100 (k = 95)
        _case("rank_n20", _points((1, 1, 70), [(2 * i + 2, 0, 0) for i in range(20)]), _points((1, 1, 70), [(0, 0, 0)]), ISO,
              n_ab=20, p95_um_ab=38_000),
        _case("rank_n100", _box((1, 2, 130), (10, 109), (0, 0), (0, 0)), _points((1, 2, 130), [(0, 1, 0)]), ISO, n_ab=100),
        _case("rank_n7", _points((1, 1, 70), [(3 * i + 1, 0, 0) for i in range(7)]), _points((1, 1, 70), [(0, 0, 0)]), ISO,
              n_ab=7, p95_um_ab=19_000),
        # the keys of A→B are x · ux for x = 1 … 60 (B is the voxel at x = 0): only one digit of the select varies
        _case("digit_low", _box((1, 1, 70), (1, 60), (0, 0), (0, 0)), _points((1, 1, 70), [(0, 0, 0)]), (1, 1000, 1000), varies=2),
        _case("digit_mid", _box((1, 1, 70), (1, 60), (0, 0), (0, 0)), _points((1, 1, 70), [(0, 0, 0)]), (1 << 10, 1000, 1000), varies=1),
        _case("digit_high", _box((1, 1, 70), (1, 60), (0, 0), (0, 0)), _points((1, 1, 70), [(0, 0, 0)]), (1 << 21, 1000, 1000), varies=0),
        _case("noise_50", noise_a, _noise((5, 11, 67), 0.5, 12), ANISO),
        _case("size", size_a, size_b, COPRIME, max_blocks=SIZE_MAX_BLOCKS),
    ]
    return cases


_CACHE = []


def cases():
    """The cases, built once."""
    if not _CACHE:
        _CACHE.extend(all_cases())
    return _CACHE


def ids(cs):
    return [c["name"] for c in cs]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def words(c):
    d, h, w = c["a"].shape
    return (w + 63) // 64 * h * d


INTEGER_KEYS = ("a_vox", "b_vox", "tp_vox", "fp_vox", "fn_vox", "surface_a", "surface_b", "n_ab", "max_um2_ab", "worst_ab", "sum_um_ab",
                "p95_um_ab", "found_ab", "n_ba", "max_um2_ba", "worst_ba", "sum_um_ba", "p95_um_ba", "found_ba")
JSON_KEYS = ("width", "height", "depth", "compare_spacing_um", "reference") + INTEGER_KEYS + (
    "dice", "jaccard", "sensitivity", "precision", "volume_a_mm3", "volume_b_mm3", "volume_diff_mm3", "hausdorff_mm", "hd95_mm",
    "msd_ab_mm", "msd_ba_mm", "assd_mm")


def swapped(r):
    """The record of compare(B, A) from that of compare(A, B)."""
    s = {"a_vox": r["b_vox"], "b_vox": r["a_vox"], "tp_vox": r["tp_vox"], "fp_vox": r["fn_vox"], "fn_vox": r["fp_vox"],
         "surface_a": r["surface_b"], "surface_b": r["surface_a"]}
    for k in ("n", "max_um2", "worst", "sum_um", "p95_um", "found"):
        s[k + "_ab"], s[k + "_ba"] = r[k + "_ba"], r[k + "_ab"]
    return s
