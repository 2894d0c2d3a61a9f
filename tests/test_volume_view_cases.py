"""The inputs of volume_view_cases have the properties they are there for (CPU, NumPy only)."""
import numpy as np
import pytest

import volume_view_cases as vc

CASES = {c["id"]: c for c in vc.all_cases()}


def test_ids_are_unique_and_sizes_small():
    cases = vc.all_cases()
    assert len({c["id"] for c in cases}) == len(cases) == len(CASES)
    for c in cases:
        assert sorted(c["raw"].shape) <= sorted(vc.MAX_SHAPE) and c["raw"].size <= 12 * 40 * 130, c["id"]
        assert c["raw"].dtype == np.uint16 and c["mask"].dtype == np.uint8 and set(np.unique(c["mask"])) <= {0, 1}, c["id"]
        assert c["why"]


def test_cases_are_deterministic():
    a, b = vc.all_cases(), vc.all_cases()
    for x, y in zip(a, b):
        assert x["id"] == y["id"] and np.array_equal(x["raw"], y["raw"]) and np.array_equal(x["mask"], y["mask"])


@pytest.mark.parametrize("n", vc.WORD_EDGES)
def test_word_edges(n):
    cw, ch = CASES[f"w{n}"], CASES[f"h{n}"]
    assert cw["raw"].shape[2] == n and ch["raw"].shape[1] == n
    # the last column (row) is set on every plane, so the last valid bit of the last word of the axial and
    # coronal (sagittal) rows is 1 in the plane views and in the shadows
    assert cw["mask"][:, :, n - 1].all() and ch["mask"][:, n - 1, :].all()
    if n > 1:
        assert not cw["mask"].all() and not ch["mask"].all()


def test_shapes_and_points():
    assert CASES["one_plane"]["raw"].shape[0] == 1 and CASES["one_plane"]["tensor_only"]
    assert CASES["one_row"]["raw"].shape[1] == 1 and CASES["one_row"]["tensor_only"]
    assert CASES["d2"]["raw"].shape[0] == 2 and not CASES["d2"]["tensor_only"]
    d, h, w = CASES["at_origin"]["raw"].shape
    assert CASES["at_origin"]["at"] == (0, 0, 0) and CASES["at_far_corner"]["at"] == (w - 1, h - 1, d - 1)
    assert CASES["at_far_corner"]["raw"].shape == (d, h, w) and CASES["at_centre"]["at"] == "centre"
    # the projection grid of the largest shape has more than one workgroup along every axis (128 × 16 × 8)
    d, h, w = CASES["plane_maxima"]["raw"].shape
    assert w > 128 and h > 16 and d > 8


def test_formats():
    c = CASES["i16"]
    v = vc.stored_values(c)
    assert c["type"] == "i16" and v.min() < 0 < v.max()
    for name in ("u12_garbage", "i12_garbage"):
        c = CASES[name]
        assert c["stored_bits"] == 12 and ((c["raw"] >> 12) != 0).all()  # the garbage bits are really set, on every sample
        v = vc.stored_values(c)
        assert (v < 4096).all() and (v.min() < 0) == (c["type"] == "i16")
    c = CASES["u8"]
    assert c["type"] == "u8" and c["stored_bits"] == 8 and c["raw"].max() == 255
    assert CASES["inverted"]["inverted"] and CASES["inverted_i16"]["inverted"] and CASES["inverted_i16"]["type"] == "i16"
    # an inverted projection differs from the plain one
    k = CASES["inverted"]["raw"]
    assert (k.min(axis=0) != k.max(axis=0)).any()


def test_masks():
    assert not CASES["empty"]["mask"].any() and CASES["full"]["mask"].all()
    m = CASES["corners"]["mask"]
    d, h, w = m.shape
    assert m.sum() == 2 and m[0, 0, 0] and m[-1, -1, -1]
    assert not m[(d - 1) // 2, (h - 1) // 2, (w - 1) // 2]  # the box centre is outside the mask
    m = CASES["faces"]["mask"]
    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and m[:, :, 0].any() and m[:, :, -1].any()
    m = CASES["off_centre"]["mask"]
    zs, ys, xs = np.nonzero(m)
    p = ((xs.min() + xs.max()) // 2, (ys.min() + ys.max()) // 2, (zs.min() + zs.max()) // 2)
    d, h, w = m.shape
    assert p != (w // 2, h // 2, d // 2) and all(a != b for a, b in zip(p, (w // 2, h // 2, d // 2)))


def test_reductions():
    for name, plane in (("max_first", 0), ("max_last", -1)):
        k = CASES[name]["raw"].astype(np.int32)
        top = k.max(axis=0)
        assert (k[plane] == top).all()
        rest = np.delete(k, plane % k.shape[0], axis=0)
        assert (rest < top).all()  # attained on that plane only
        assert (np.sort(rest, axis=0)[-1] == np.sort(rest, axis=0)[-2]).any()  # ties below it
    k = CASES["plane_maxima"]["raw"].astype(np.int32)
    per_plane = k.reshape(k.shape[0], -1).max(axis=1)
    assert len(set(per_plane.tolist())) > k.shape[0] // 2 and per_plane.argmax() == 7
    mip = k.max(axis=0)
    assert all((mip != k[z]).any() for z in range(k.shape[0]))  # the MIP differs from every single plane
    assert (k[: 7].max(axis=0) != mip).any()  # stopping before plane 7 is wrong
    k = CASES["edge_maxima"]["raw"].astype(np.int32)
    assert (k.max(axis=1) == k[:, -1, :]).all() and (k.max(axis=2) == k[:, :, -1]).all()
    assert (k[:, 0, 1:-1] > k[:, 1:-1, 1:-1].max(axis=1)).all()
