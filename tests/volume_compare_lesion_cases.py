"""Shared cases of the lesion-wise comparison tests (nm03/volume_compare_lesions.h, K18): pairs of masks as uint8
[D, H, W] and what each case claims about itself — the component counts of both masks at both connectivities, whether a
side has more than 64 components, whether the reporting order or a best partner rests on a tie — checked with SciPy by
test_volume_compare_lesion_cases.py, so that a later edit of a mask cannot empty a test. Every comparison made with
them is == on integers and text."""
import numpy as np

import volume_compare_cases as cc

# The kernels' constants (src/kernels/k18_volume_compare_lesions.hip): 256 words per workgroup, at most 1024
# workgroups in the join launch. "size" (130 × 40 × 24: 3 · 40 · 24 = 2880 words, 12 blocks of 256) runs at
# max_blocks = 1 (12 trips of the join's strided loop), 5 (3 trips, the last one partial) and the default (1 trip).
WORDS_PER_BLOCK = 256
MAX_BLOCKS = 1024
SIZE_MAX_BLOCKS = (1, 5, None)
MAX_LESIONS = 64
NS = (1, 2, 64)  # the N every case runs at

_points, _box, _ball, _noise = cc._points, cc._box, cc._ball, cc._noise


def _case(name, a, b, counts, **claims):
    """counts = (lesions_a at c = 6, lesions_b at 6, lesions_a at 26, lesions_b at 26)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    b = np.ascontiguousarray(b, dtype=np.uint8)
    assert a.shape == b.shape and a.ndim == 3, name
    a.setflags(write=False)
    b.setflags(write=False)
    c = {"name": name, "a": a, "b": b, "counts": tuple(counts), "exceeds": False, "size_tie": False, "best_tie": False,
         "max_blocks": (None,)}
    c.update(claims)
    return c


def _runs(shape, runs):
    """runs: (z, y, x0, x1) inclusive."""
    m = np.zeros(shape, np.uint8)
    for z, y, x0, x1 in runs:
        m[z, y, x0:x1 + 1] = 1
    return m


def _width_case(w):
    # Row 0: a run of A through every word edge of the row while B's runs end inside the words, and one of B's that
    # starts in the word before the edge and ends just behind it. Row 2: the converse. Row 4: both cross the edges,
    # from different starts. The rows are two apart, so each run is a component at either connectivity.
    shape = (2, 5, w)
    long_run = (3, w - 1)
    row = [(x0, min(x1, w - 1)) for x0, x1 in ((0, 1), (10, 20), (61, 66), (70, 75), (120, 125), (127, 129)) if x0 < w]
    a = _runs(shape, [(0, 0) + long_run] + [(0, 2, x0, x1) for x0, x1 in row] + [(0, 4, 1, w - 1)])
    b = _runs(shape, [(0, 0, x0, x1) for x0, x1 in row] + [(0, 2) + long_run] + [(0, 4, 0, w - 3)])
    n = len(row)
    return _case(f"width_{w}", a, b, (n + 2, n + 2, n + 2, n + 2), width=w, size_tie=w in (63, 130))


def _lattice():
    # More than 64 components on each side. A: 108 single voxels two apart in plane 0, a box in plane 2 and five single
    # voxels in the last row of plane 2; B: a box in plane 0 over A's late single voxels, 108 single voxels in plane 2
    # of which the late ones lie in A's box, and the same five single voxels. At N = 64 each side reports its box and
    # its first 63 single voxels, so the box of one side meets unreported single voxels of the other (row and column
    # N of the table), and the five shared voxels are unreported on both sides (cell [N][N]).
    shape = (3, 20, 70)
    singles_a = [(2 * i, 2 * j, 0) for j in range(9) for i in range(12)]
    singles_b = [(30 + 2 * i, 2 * j, 2) for j in range(9) for i in range(12)]
    shared = [(2 * i, 19, 2) for i in range(5)]
    a = _points(shape, singles_a + shared) | _box(shape, (30, 50), (12, 18), (2, 2))
    b = _points(shape, singles_b + shared) | _box(shape, (0, 22), (12, 16), (0, 0))
    return _case("lattice", a, b, (114, 114, 114, 114), exceeds=True, size_tie=True)


def all_cases():
    small = (4, 6, 70)
    # worked example 2 of the header: the row at c = 6
    row_a = _points((1, 1, 12), [(x, 0, 0) for x in (0, 1, 2, 4, 5, 6, 9)])
    row_b = _points((1, 1, 12), [(x, 0, 0) for x in (2, 3, 4, 11)])
    # a diagonal-only contact on both sides: the voxels of each pair share a corner (A) or an edge (B) only
    diag_a = _points((4, 4, 8), [(1, 1, 1), (2, 2, 2), (6, 0, 0)])
    diag_b = _points((4, 4, 8), [(2, 2, 2), (3, 3, 2), (6, 0, 0), (6, 1, 1)])
    # one lesion of A over three of B
    merge_a = _box(small, (5, 66), (1, 4), (1, 2))
    merge_b = _box(small, (8, 12), (2, 3), (1, 1)) | _box(small, (30, 31), (0, 5), (2, 2)) | _box(small, (60, 69), (4, 5), (1, 3))
    # a best-partner tie: B's bar meets two boxes of A in two voxels each; the boxes differ in size
    tie_a = _box(small, (10, 13), (2, 2), (1, 1)) | _box(small, (20, 25), (2, 3), (1, 1))
    tie_b = _box(small, (12, 21), (2, 2), (1, 1))
    equal = _noise(small, 0.3, 5)
    sup = _box(small, (2, 40), (1, 4), (0, 2)) | _points(small, [(60, 0, 3), (62, 5, 0)])
    sub = _box(small, (4, 9), (2, 3), (1, 1)) | _box(small, (20, 30), (1, 2), (2, 2)) | _points(small, [(60, 0, 3)])
    size = cc.case("size")
    cases = [
        _case("worked_boxes", cc.case("worked_boxes")["a"], cc.case("worked_boxes")["b"], (1, 2, 1, 2)),
        _case("worked_row", row_a, row_b, (3, 2, 3, 2), size_tie=True, best_tie=True),
    ]
    cases += [_width_case(w) for w in (63, 64, 65, 130)]
    cases += [
        _case("diagonal", diag_a, diag_b, (3, 4, 2, 2), size_tie=True),
        _case("merge", merge_a, merge_b, (1, 3, 1, 3)),
        _case("split", merge_b, merge_a, (3, 1, 3, 1)),
        # the two boxes share exactly the voxels x = 5 of one row
        _case("touch_one", _box(small, (0, 5), (2, 2), (1, 1)), _box(small, (5, 9), (2, 2), (1, 1)), (1, 1, 1, 1), tp_vox=1),
        _lattice(),
        # three lesions of two voxels each: the order rests on the first voxel
        _case("equal_areas", _runs(small, [(3, 5, 60, 61), (0, 0, 10, 11), (1, 3, 30, 31)]),
              _runs(small, [(0, 0, 11, 12), (3, 5, 59, 60), (2, 2, 1, 2)]), (3, 3, 3, 3), size_tie=True),
        _case("best_tie", tie_a, tie_b, (2, 1, 2, 1), best_tie=True),
        _case("a_empty", np.zeros(small, np.uint8), equal, (0, 160, 0, 1), exceeds=True, size_tie=True),
        _case("b_empty", equal, np.zeros(small, np.uint8), (160, 0, 1, 0), exceeds=True, size_tie=True),
        _case("both_empty", np.zeros(small, np.uint8), np.zeros(small, np.uint8), (0, 0, 0, 0)),
        _case("equal", equal, equal, (160, 160, 1, 1), exceeds=True, size_tie=True),
        _case("subset", sub, sup, (3, 3, 3, 3), subset=True, size_tie=True),
        _case("noise_50", cc.case("noise_50")["a"], cc.case("noise_50")["b"], (70, 62, 1, 1), exceeds=True, size_tie=True),
        _case("size", size["a"], size["b"], (271, 232, 266, 226), exceeds=True, size_tie=True, max_blocks=SIZE_MAX_BLOCKS),
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


TOTAL_KEYS = ("lesions_a", "hit_a", "multi_a", "lesions_b", "hit_b", "multi_b")
RECORD_KEYS = ("voxels", "first", "overlap_vox", "partners_reported", "overlap_other_vox", "multi", "best", "best_overlap_vox")
DICT_KEYS = ("connectivity", "max_lesions") + TOTAL_KEYS + ("a_lesions", "b_lesions", "table")
JSON_LESION_KEYS = ("lesions_connectivity", "lesions_max") + TOTAL_KEYS + ("lesion_sensitivity", "lesion_precision", "lesion_f1",
                                                                             "a_lesions", "b_lesions")
JSON_RECORD_KEYS = RECORD_KEYS + ("coverage", "best_dice")
CSV_LESION_COLUMNS = TOTAL_KEYS + ("lesion_sensitivity", "lesion_precision", "lesion_f1")
TABLE_COLUMNS = ("patient", "side", "lesion", "voxels", "first_x", "first_y", "first_z", "overlap_vox", "partners_reported",
                 "overlap_other_vox", "multi", "best", "best_overlap_vox")


def plain(r):
    """A result dict with the table as nested lists (an int64 array or tensor otherwise), for ==."""
    r = dict(r)
    t = r["table"]
    r["table"] = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).astype(np.int64).tolist()
    return r


def swapped(r):
    """The record of compare(B, A) from that of compare(A, B): the sides exchanged, the table transposed."""
    r = plain(r)
    s = {"connectivity": r["connectivity"], "max_lesions": r["max_lesions"]}
    for k in ("lesions", "hit", "multi"):
        s[k + "_a"], s[k + "_b"] = r[k + "_b"], r[k + "_a"]
    s["a_lesions"], s["b_lesions"] = r["b_lesions"], r["a_lesions"]
    s["table"] = np.asarray(r["table"], dtype=np.int64).T.tolist()
    return {k: s[k] for k in DICT_KEYS}
