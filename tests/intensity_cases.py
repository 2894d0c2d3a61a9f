"""Shared case builders of the --measure-intensity tests (CPU and GPU): deterministic, fixed seeds. A
case is (name, mask bool, raw uint16 storage, pixel_type, stored_bits); 2D arrays are [H, W], 3D
[D, H, W]. They are the smallest shapes at which the K11 kernels can still go wrong."""
import functools

import numpy as np

PERCENTILES = (10, 25, 50, 75, 90)
INT_KEYS = ("raw_sum_sq",) + tuple(f"raw_p{p}" for p in PERCENTILES)
DOUBLE_KEYS = ("std", "p10", "p25", "median", "p75", "p90", "iqr")


def _rng(seed):
    return np.random.default_rng(seed)


def _store(values, pixel_type, stored_bits, junk_seed=None):
    """Signed or unsigned values → 16-bit storage; with junk_seed the bits above stored_bits are noise."""
    v = np.asarray(values, dtype=np.int64)
    s = (v & ((1 << stored_bits) - 1)).astype(np.uint16)
    if junk_seed is not None and stored_bits < 16:
        junk = _rng(junk_seed).integers(0, 1 << (16 - stored_bits), size=s.shape).astype(np.uint16)
        s = s | (junk << np.uint16(stored_bits))
    return s


def _random(w, h, seed, density=0.7, lo=0, hi=65536, pixel_type="u16", stored_bits=16, junk=False):
    r = _rng(seed)
    mask = r.random((h, w)) < density
    raw = _store(r.integers(lo, hi, size=(h, w)), pixel_type, stored_bits, seed + 1 if junk else None)
    return mask, raw, pixel_type, stored_bits


def _n_pixels(n, seed, w=70, h=5):
    """Exactly n mask pixels with distinct values; every other sample is noise that must not count."""
    r = _rng(seed)
    mask = np.zeros(h * w, bool)
    mask[r.choice(h * w, size=n, replace=False)] = True
    raw = r.permutation(65536)[:h * w].astype(np.uint16)
    return mask.reshape(h, w), raw.reshape(h, w), "u16", 16


def _placed(values, seed, w=70, h=5, fill=7):
    """A mask of len(values) pixels holding exactly `values` (shuffled)."""
    r = _rng(seed)
    vals = np.asarray(values, dtype=np.int64)
    mask = np.zeros(h * w, bool)
    pos = r.choice(h * w, size=vals.size, replace=False)
    mask[pos] = True
    raw = np.full(h * w, fill, np.int64)
    raw[pos] = r.permutation(vals)
    return mask.reshape(h, w), raw.astype(np.uint16).reshape(h, w), "u16", 16


def _clusters(n_low, n_high, seed):
    """Two clusters on both sides of the boundary between high bytes 0x10 and 0x11: the low one ends on
    0x10FF, the last key of its bin, the high one starts on 0x1100, the first key of the next."""
    r = _rng(seed)
    low = np.concatenate([r.integers(0x1080, 0x10FF, size=n_low - 1), [0x10FF]])
    high = np.concatenate([[0x1100], r.integers(0x1101, 0x1180, size=n_high - 1)])
    return _placed(np.concatenate([low, high]), seed + 1, w=70, h=5)


def _all_equal():
    return np.ones((40, 130), bool), np.full((40, 130), 1234, np.uint16), "u16", 16


def _full_65535():
    return np.ones((512, 512), bool), np.full((512, 512), 65535, np.uint16), "u16", 16


def _low_byte_only():
    m, raw, t, b = _random(130, 9, 31)
    return m, ((raw & np.uint16(0xFF)) | np.uint16(0x4200)), t, b


def _high_byte_only():
    m, raw, t, b = _random(130, 9, 32)
    return m, ((raw & np.uint16(0xFF00)) | np.uint16(0x37)), t, b


def _empty():
    _, raw, t, b = _random(70, 5, 33)
    return np.zeros((5, 70), bool), raw, t, b


@functools.lru_cache(maxsize=None)
def cases_2d():
    c = [
        ("1x1", *_random(1, 1, 1, density=2.0)),
        ("65x2", *_random(65, 2, 2)),
        ("64x3", *_random(64, 3, 3)),
        ("70x5", *_random(70, 5, 4)),
        ("256x300_second_trip", *_random(256, 300, 5)),
        ("4096x3_widest_rows", *_random(4096, 3, 6, density=0.3)),  # 64 words a row, the engine's largest width
        ("empty", *_empty()),
    ]
    c += [(f"n{n}", *_n_pixels(n, 10 + n)) for n in (1, 2, 3, 4, 20, 100)]
    c += [
        ("all_equal", *_all_equal()),
        ("low_byte_only", *_low_byte_only()),
        ("high_byte_only", *_high_byte_only()),
        # n = 4: ranks 1, 1, 2, 3, 4 — p50 is the last sample of bin 0x10, p75 the first of bin 0x11
        ("clusters_2_2", *_clusters(2, 2, 40)),
        # n = 100: rank 50 is the last sample of bin 0x10 / the first sample of bin 0x11
        ("clusters_50_50", *_clusters(50, 50, 42)),
        ("clusters_49_51", *_clusters(49, 51, 44)),
        ("clusters_25_75", *_clusters(25, 75, 46)),
        ("u16_high", *_random(70, 5, 50, lo=32768, hi=65536)),
        ("i16_16", *_random(130, 7, 51, lo=-32768, hi=32768, pixel_type="i16", stored_bits=16)),
        ("i16_12_junk", *_random(130, 7, 52, lo=-2048, hi=2048, pixel_type="i16", stored_bits=12, junk=True)),
        ("u16_12_junk", *_random(130, 7, 53, lo=0, hi=4096, pixel_type="u16", stored_bits=12, junk=True)),
        ("u8", *_random(70, 5, 54, lo=0, hi=256, pixel_type="u8", stored_bits=8)),
        ("full_512_65535", *_full_65535()),
    ]
    return tuple(c)


def _volume(w, h, d, seed, density=0.4, **kw):
    r = _rng(seed)
    mask = r.random((d, h, w)) < density
    pt, bits = kw.get("pixel_type", "u16"), kw.get("stored_bits", 16)
    raw = _store(r.integers(kw.get("lo", 0), kw.get("hi", 65536), size=(d, h, w)), pt, bits)
    return mask, raw, pt, bits


def _single_last_voxel():
    mask, raw, pt, bits = _volume(70, 9, 6, 63)
    mask[:] = False
    mask[-1, -1, -1] = True  # the last word of the last plane
    return mask, raw, pt, bits


def _empty_volume():
    mask, raw, pt, bits = _volume(70, 9, 6, 64)
    return np.zeros_like(mask), raw, pt, bits


@functools.lru_cache(maxsize=None)
def cases_3d():
    return (
        ("70x9x40_three_workgroups", *_volume(70, 9, 40, 60)),
        ("256x64x20", *_volume(256, 64, 20, 61)),
        ("i16_70x9x40", *_volume(70, 9, 40, 62, lo=-32768, hi=32768, pixel_type="i16")),
        ("homogeneous_70x9x40", *((lambda m, r, p, b: (m, np.full_like(r, 4660), p, b))(*_volume(70, 9, 40, 65, density=0.9)))),
        ("single_last_voxel", *_single_last_voxel()),
        ("empty", *_empty_volume()),
    )


def ids(cases):
    return [c[0] for c in cases]
