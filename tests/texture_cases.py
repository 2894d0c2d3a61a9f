"""Shared case builders of the --measure-texture tests (CPU and GPU): deterministic, fixed seeds. A case
is (name, mask bool, raw uint16 storage, pixel_type, stored_bits, levels); 2D arrays are [H, W], 3D
[D, H, W]. They are the smallest shapes at which the K12 kernels can still go wrong."""
import functools

import numpy as np

from intensity_cases import _store

INT_KEYS = ("glcm_levels", "glcm_pairs", "glcm_nonzero", "glcm_max_count", "glcm_sum_abs_d", "glcm_sum_d2", "glcm_sum_sq")
DOUBLE_KEYS = tuple("glcm_" + k for k in (
    "joint_max", "joint_avg", "joint_var", "joint_entropy", "asm", "contrast", "dissimilarity", "inv_diff", "inv_diff_moment",
    "correlation", "autocorrelation", "cluster_tendency", "cluster_shade", "cluster_prominence", "sum_entropy", "diff_entropy"))
NEW_COLUMNS = list(INT_KEYS + DOUBLE_KEYS)
HEAD_KEYS = ("levels", "key_lo", "key_hi", "samples", "pairs")

HARALICK = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint16)
HARALICK_MERGED = np.array([[16, 4, 6, 0], [4, 12, 5, 0], [6, 5, 12, 6], [0, 0, 6, 2]], np.uint32)
HARALICK_EAST = np.array([[4, 2, 1, 0], [2, 4, 0, 0], [1, 0, 6, 1], [0, 0, 1, 2]], np.uint32)


def _rng(seed):
    return np.random.default_rng(seed)


def _random(shape, seed, density=0.7, lo=0, hi=65536, pixel_type="u16", stored_bits=16, junk=False, levels=32):
    r = _rng(seed)
    mask = r.random(shape) < density
    raw = _store(r.integers(lo, hi, size=shape), pixel_type, stored_bits, seed + 1 if junk else None)
    return mask, raw, pixel_type, stored_bits, levels


def _full(shape, seed, levels=32):
    return _random(shape, seed, density=2.0, levels=levels)


def _masked(mask, seed, levels=32):
    raw = _rng(seed).integers(0, 65536, size=mask.shape).astype(np.uint16)
    return mask, raw, "u16", 16, levels


def _isolated():
    """A checkerboard of 4: every second pixel of every second row, no two mask pixels adjacent."""
    m = np.zeros((9, 70), bool)
    m[::2, ::2] = True
    return _masked(m, 31)


def _checkerboard():
    yy, xx = np.mgrid[0:9, 0:70]
    return _masked((yy + xx) % 2 == 0, 32)


def _column_stripes():
    m = np.zeros((9, 70), bool)
    m[:, ::2] = True
    return _masked(m, 33)


def _row_stripes():
    m = np.zeros((9, 70), bool)
    m[::2, :] = True
    return _masked(m, 34)


def _bin_edges(levels=8):
    """Samples exactly at lo + k · (hi − lo) / Ng and one below each, in a full 2-row mask."""
    lo, hi = 1000, 1000 + 8 * 977
    edges = [lo + k * (hi - lo) // levels for k in range(levels + 1)]
    vals = sorted(set(edges + [e - 1 for e in edges[1:]]))
    vals = np.array((vals * 8)[:2 * 66], np.int64)
    return np.ones((2, 66), bool), _rng(35).permutation(vals).astype(np.uint16).reshape(2, 66), "u16", 16, levels


def _two_values():
    raw = np.where(_rng(36).random((7, 70)) < 0.5, 17, 40000).astype(np.uint16)
    return _rng(37).random((7, 70)) < 0.8, raw, "u16", 16, 32


def _ramp():
    raw = np.tile(np.arange(130, dtype=np.uint16), (4, 1))
    return np.ones((4, 130), bool), raw, "u16", 16, 16


def _homogeneous_512():
    return np.ones((512, 512), bool), np.full((512, 512), 30000, np.uint16), "u16", 16, 32


HOMOGENEOUS_512_CELL = 2 * (511 * 512 + 512 * 511 + 2 * 511 * 511)


@functools.lru_cache(maxsize=None)
def cases_2d():
    r130 = _random((9, 130), 50)
    c = [
        ("1x1", *_full((1, 1), 1)),
        ("2x1", *_full((1, 2), 2)),
        ("1x2", *_full((2, 1), 3)),
        ("2x2", *_full((2, 2), 4)),
        ("haralick_4x4", np.ones((4, 4), bool), HARALICK.copy(), "u16", 16, 4),
        ("64x2", *_full((2, 64), 5)),
        ("65x2", *_full((2, 65), 6)),
        ("128x3", *_full((3, 128), 7)),
        ("70x5", *_random((5, 70), 8)),
        ("256x300", *_random((300, 256), 9, density=0.6)),
        ("4096x3", *_random((3, 4096), 10)),
        ("3x1100", *_random((1100, 3), 11)),
        ("empty", np.zeros((5, 70), bool), _rng(12).integers(0, 65536, size=(5, 70)).astype(np.uint16), "u16", 16, 32),
        ("isolated", *_isolated()),
        ("checkerboard", *_checkerboard()),
        ("column_stripes", *_column_stripes()),
        ("row_stripes", *_row_stripes()),
        ("all_equal", np.ones((6, 130), bool), np.full((6, 130), 1234, np.uint16), "u16", 16, 32),
        ("two_values", *_two_values()),
        ("bin_edges", *_bin_edges()),
        ("ramp", *_ramp()),
        ("i16_16", *_random((7, 70), 20, lo=-32768, hi=32768, pixel_type="i16")),
        ("i16_12_junk", *_random((7, 70), 21, lo=-2048, hi=2048, pixel_type="i16", stored_bits=12, junk=True)),
        ("u16_12_junk", *_random((7, 70), 22, lo=0, hi=4096, stored_bits=12, junk=True)),
        ("u8", *_random((7, 70), 23, lo=0, hi=256, pixel_type="u8", stored_bits=8)),
    ]
    for lv in (2, 8, 16, 63, 64):
        c.append((f"levels_{lv}", *r130[:4], lv))
    c.append(("full_512_homogeneous", *_homogeneous_512()))
    return tuple(c)


@functools.lru_cache(maxsize=None)
def cases_3d():
    _, mask2, raw2, ptype2, bits2, lv2 = next(c for c in cases_2d() if c[0] == "70x5")
    last = np.zeros((3, 5, 70), bool)
    last[-1, -1, -1] = True
    return (
        ("2x2x2", *_full((2, 2, 2), 60)),
        ("1x1x2", *_full((2, 1, 1), 61)),
        ("d1_equals_2d", mask2[None].copy(), raw2[None].copy(), ptype2, bits2, lv2),
        ("70x9x40", *_random((40, 9, 70), 62)),
        ("130x5x3", *_random((3, 5, 130), 63)),
        ("i16_70x9x40", *_random((40, 9, 70), 64, lo=-32768, hi=32768, pixel_type="i16")),
        ("homogeneous_70x9x40", np.ones((40, 9, 70), bool), np.full((40, 9, 70), 777, np.uint16), "u16", 16, 32),
        ("single_last_voxel", *_masked(last, 65)),
        ("empty", np.zeros((3, 5, 70), bool), _rng(66).integers(0, 65536, size=(3, 5, 70)).astype(np.uint16), "u16", 16, 32),
        ("levels_64_70x9x12", *_random((12, 9, 70), 67, levels=64)),
    )


def ids(cases):
    return [c[0] for c in cases]


def same(a, b):
    """Two texture record dicts compare equal: the header integers and the matrix, with ==."""
    return (set(a) == set(b) and all(a[k] == b[k] for k in HEAD_KEYS) and a["glcm"].dtype == b["glcm"].dtype
            and a["glcm"].shape == b["glcm"].shape and bool((a["glcm"] == b["glcm"]).all()))
