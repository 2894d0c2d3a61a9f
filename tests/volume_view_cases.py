"""Inputs of the volume-view tests (test_volume_view_cases.py and test_volume_views.py on the CPU,
test_gpu_volume_views.py on the GPU; not a conftest): small deterministic volumes for K14 and its golden
model, each with the property it is there for (test_volume_view_cases.py asserts every one of them on the
inputs themselves). Every volume is at most 130 × 40 × 12 — with the axes in any order, since the transposed
word-edge cases put the long side in h.

A case is a dict: id, raw (uint16 [d, h, w] stored words), mask (uint8 [d, h, w], the "dilated" mask), type,
stored_bits, inverted, at ("mask" | "centre" | (x, y, z)), tensor_only (d = 1 or h = 1: below what the 3D
pipeline takes, so the tensor op and the golden model only) and why."""
import numpy as np

MAX_SHAPE = (12, 40, 130)  # d, h, w
WORD_EDGES = (1, 63, 64, 65, 130)


def _rng(seed):
    return np.random.default_rng(seed)


def noise(shape, seed, lo=0, hi=4096):
    return _rng(seed).integers(lo, hi, size=shape, dtype=np.int64).astype(np.uint16)


def blob(shape, seed, fill=0.15):
    """A random mask with a solid box in it, away from the faces where the shape allows."""
    d, h, w = shape
    m = (_rng(seed).random(shape) < fill).astype(np.uint8)
    m[d // 3:max(d // 3 + 1, 2 * d // 3), h // 4:max(h // 4 + 1, h // 2), w // 4:max(w // 4 + 1, 3 * w // 4)] = 1
    return m


def case(id, raw, mask, why, type="u16", stored_bits=16, inverted=False, at="mask", tensor_only=False):
    raw = np.ascontiguousarray(raw, dtype=np.uint16)
    mask = np.ascontiguousarray(mask, dtype=np.uint8)
    assert raw.shape == mask.shape and all(a <= b for a, b in zip(sorted(raw.shape), sorted(MAX_SHAPE))), id
    raw.setflags(write=False)
    mask.setflags(write=False)
    return dict(id=id, raw=raw, mask=mask, type=type, stored_bits=stored_bits, inverted=inverted, at=at,
                tensor_only=tensor_only, why=why)


def width_cases():
    """w = 1, 63, 64, 65, 130: the word edges of the axial and coronal bit layouts; the same values for h in
    a transposed case each: the word edges of the sagittal layout (these volumes are narrow: w = 5)."""
    out = []
    for i, w in enumerate(WORD_EDGES):
        shape = (5, 7, w)
        m = blob(shape, 100 + i, 0.3)
        m[:, :, w - 1] = 1  # the last column of the last word is set
        out.append(case(f"w{w}", noise(shape, 10 + i), m, f"width {w}: last valid bit of the last word of a row"))
    for i, h in enumerate(WORD_EDGES):
        shape = (5, h, 5)
        m = blob(shape, 200 + i, 0.3)
        m[:, h - 1, :] = 1
        out.append(case(f"h{h}", noise(shape, 20 + i), m, f"height {h}: last valid bit of the sagittal views' last word"))
    return out


def format_cases():
    shape = (6, 20, 70)
    out = []
    # signed 16-bit with negative samples
    v = _rng(31).integers(-2000, 2000, size=shape).astype(np.int16)
    out.append(case("i16", v.view(np.uint16), blob(shape, 32), "signed samples, negative ones among them", type="i16"))
    # 12 stored bits, random bits above bit 11
    lo = noise(shape, 33, 0, 4096)
    hi = (_rng(34).integers(1, 16, size=shape).astype(np.uint16) << 12).astype(np.uint16)
    out.append(case("u12_garbage", lo | hi, blob(shape, 35), "12 stored bits with garbage above bit 11", stored_bits=12))
    # signed 12 bits with garbage: sign extension from bit 11
    out.append(case("i12_garbage", lo | hi, blob(shape, 36), "signed 12 stored bits with garbage above bit 11", type="i16",
                    stored_bits=12))
    # 8-bit data, held as 16-bit words with 8 stored bits
    out.append(case("u8", noise(shape, 37, 0, 256), blob(shape, 38), "8-bit samples", type="u8", stored_bits=8))
    # negative slope: the smallest key is the brightest pixel
    out.append(case("inverted", noise(shape, 39), blob(shape, 40), "negative rescale slope: the smallest key wins", inverted=True))
    out.append(case("inverted_i16", v.view(np.uint16), blob(shape, 41), "negative slope on signed samples", type="i16",
                    inverted=True))
    return out


def mask_cases():
    shape = (7, 18, 67)
    d, h, w = shape
    out = []
    out.append(case("empty", noise(shape, 50), np.zeros(shape, np.uint8), "an empty mask: no box, P falls back to the centre"))
    out.append(case("full", noise(shape, 51), np.ones(shape, np.uint8), "a mask that fills the volume"))
    m = np.zeros(shape, np.uint8)
    m[0, 0, 0] = m[d - 1, h - 1, w - 1] = 1
    out.append(case("corners", noise(shape, 52), m, "two voxels in opposite corners: the box centre is outside the mask"))
    m = np.zeros(shape, np.uint8)
    m[0, 5, 9] = m[d - 1, 6, 9] = m[3, 0, 20] = m[3, h - 1, 21] = m[2, 9, 0] = m[4, 9, w - 1] = 1
    out.append(case("faces", noise(shape, 53), m, "a mask touching all six frame faces"))
    m = np.zeros(shape, np.uint8)
    m[1:3, 2:5, 3:9] = 1
    out.append(case("off_centre", noise(shape, 54), m, "P from the mask differs from the centre"))
    return out


def reduction_cases():
    shape = (12, 40, 130)  # the largest: the projection grid has 2 × 3 × 2 workgroups (128 columns, 16 rows, 8 planes each)
    d, h, w = shape
    out = []
    # the maximum of every column attained on the first plane only / the last plane only, with ties below it
    base = noise(shape, 60, 0, 8)  # many ties
    first = base.copy()
    first[0] = 1000
    out.append(case("max_first", first, blob(shape, 61), "the z-maximum on the first plane only (ties below it)"))
    last = base.copy()
    last[d - 1] = 1000
    out.append(case("max_last", last, blob(shape, 62), "the z-maximum on the last plane only"))
    # per-plane maxima that differ and rise with z, then fall: a projection that stops early is wrong
    ramp = noise(shape, 63, 0, 100)
    for z in range(d):
        ramp[z, (3 * z) % h, (11 * z) % w] = 2000 + 10 * (z if z < 8 else 15 - z)
    out.append(case("plane_maxima", ramp, blob(shape, 64), "every plane has its own maximum, the largest on plane 7"))
    # maxima in the first / last row and column: the ends of the y and x reductions
    edge = noise(shape, 65, 0, 50)
    edge[:, 0, :] = 900
    edge[:, h - 1, :] = 901
    edge[:, :, 0] = np.maximum(edge[:, :, 0], 950)
    edge[:, :, w - 1] = 951
    out.append(case("edge_maxima", edge, blob(shape, 66), "row and column maxima on the first and last row / column"))
    return out


def shape_cases():
    out = []
    out.append(case("one_plane", noise((1, 9, 70), 70), blob((1, 9, 70), 71, 0.3), "one plane", tensor_only=True))
    out.append(case("one_row", noise((5, 1, 70), 72), blob((5, 1, 70), 73, 0.3), "one row", tensor_only=True))
    out.append(case("d2", noise((2, 11, 33), 74), blob((2, 11, 33), 75, 0.3), "two planes"))
    shape = (6, 13, 66)
    out.append(case("at_origin", noise(shape, 76), blob(shape, 77), "explicit point on the frame: the origin", at=(0, 0, 0)))
    out.append(case("at_far_corner", noise(shape, 78), blob(shape, 79), "explicit point on the frame: the far corner",
                    at=(65, 12, 5)))
    out.append(case("at_centre", noise(shape, 80), blob(shape, 81), "the centre of the volume, whatever the mask", at="centre"))
    return out


def all_cases():
    return width_cases() + format_cases() + mask_cases() + reduction_cases() + shape_cases()


def ids(cases):
    return [c["id"] for c in cases]


def stored_values(c):
    """int32 stored sample values of a case: masked to the stored bits, sign-extended for i16."""
    raw = c["raw"]
    sh = 16 - c["stored_bits"]
    if c["type"] == "i16":
        return ((raw.astype(np.int32) << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int32) >> sh
    return raw.astype(np.int32) & (0xFFFF >> sh)


VIEW_NAMES = ("view_axial", "view_coronal", "view_sagittal", "mip_axial", "mip_coronal", "mip_sagittal")
INT_KEYS = ("width", "height", "raw_min", "raw_max", "mask_px")


def assert_views_equal(a, b):
    """Two views dicts (ops.volume_views, reference, golden): every integer, sample and bit."""
    for k in ("width", "height", "depth", "at_mode", "inverted"):
        assert a[k] == b[k], k
    assert tuple(a["at"]) == tuple(b["at"])
    assert (None if a["mask_bbox"] is None else list(a["mask_bbox"])) == (None if b["mask_bbox"] is None else list(b["mask_bbox"]))
    assert list(a["views"]) == list(VIEW_NAMES) == list(b["views"])
    for name in VIEW_NAMES:
        va, vb = a["views"][name], b["views"][name]
        for k in INT_KEYS:
            assert va[k] == vb[k], (name, k, va[k], vb[k])
        assert va["raw"].dtype == np.uint16 and va["raw"].shape == (va["height"], va["width"]) == vb["raw"].shape, name
        assert np.array_equal(va["raw"], vb["raw"]), name + " samples"
        assert np.array_equal(va["mask"], vb["mask"]), name + " mask"
