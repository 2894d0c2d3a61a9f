"""The inputs of volume_trip_cases have the properties they are there for, so that test_gpu_volume_trips.py cannot pass
for the wrong reason (CPU; the SciPy comparison alone needs SciPy). Everything is compared with ==:
  the thickness cases     the word counts and the trips they make; the trips in which the golden background map attains
                          its maximum over the mask; golden thickness == the stated record == the SciPy-index reference
                          == the host run of the kernels' per-line functions (native.volume_thickness_words)
  the K14 cases           element and word counts against the trip thresholds, the projection grid, deep_point's z range,
                          golden == the NumPy reference
  with_bits_past_width    sets at least one bit past every width used, and unpack_bits gives the mask back"""
import numpy as np
import pytest

import volume_distance_cases as dc
import volume_mesh_cases as mc
import volume_trip_cases as tc
import volume_view_cases as vc

THICKNESS = tc.thickness_cases()
VIEWS = tc.view_cases()


@pytest.fixture(scope="module")
def background_maps(native):
    """The golden map to the background of every thickness case, computed once and shared (read-only)."""
    out = {}
    for c in THICKNESS:
        g = native.golden_volume_distance(c["mask"], list(c["um"]), True, None)
        g.setflags(write=False)
        out[c["name"]] = g
    return out


def test_kernel_constants():
    assert tc.DIST_WORDS_PER_TRIP == 4096 and tc.VV_INIT_ELEMENTS_PER_TRIP == 262144 and tc.VV_THREADS == 256
    assert len({c["name"] for c in THICKNESS}) == len(THICKNESS) and set(tc.MAP_CASES) <= {c["name"] for c in THICKNESS}
    a, b = tc.thickness_cases.__wrapped__(), tc.view_cases.__wrapped__()  # deterministic
    assert all(np.array_equal(x["mask"], y["mask"]) for x, y in zip(a, THICKNESS))
    assert all(np.array_equal(b[k]["raw"], VIEWS[k]["raw"]) and np.array_equal(b[k]["mask"], VIEWS[k]["mask"]) for k in VIEWS)


@pytest.mark.parametrize("c", THICKNESS, ids=dc.ids(THICKNESS))
def test_thickness_case_turns_the_loop(native, background_maps, c):
    shape = c["mask"].shape
    n = tc.word_count(shape)
    assert n > tc.DIST_WORDS_PER_TRIP * (c["trips"] - 1) and tc.trips(n, tc.DIST_WORDS_PER_TRIP) == c["trips"] >= 2
    assert c["mask"].size <= 137 * 64 * 64
    g = background_maps[c["name"]]
    m = c["mask"].astype(bool)
    best = int(g[m].max())
    zs, ys, xs = np.nonzero(m & (g == best))
    assert tuple(sorted(set(tc.trip_of(shape, zs, ys, xs).tolist()))) == c["attained_in"]
    x, y, z = c["want"]["inscribed_at"]
    assert best == c["want"]["inscribed_um2"] and (int(xs[0]), int(ys[0]), int(zs[0])) == (x, y, z)  # the first in raster order
    assert tc.trip_of(shape, z, y, x) == c["attained_in"][0]
    t = native.golden_volume_thickness(c["mask"], list(c["um"]))
    assert {k: t[k] for k in c["want"]} == c["want"]
    assert t["inscribed_radius_mm"] == np.sqrt(float(best)) / 1000.0 and t["thickness_mm"] == 2 * t["inscribed_radius_mm"]
    assert native.volume_thickness_words(c["mask"], list(c["um"])) == t
    pytest.importorskip("scipy.ndimage")
    from nm03_capstone_project_amd.ops import reference
    assert reference.volume_thickness(c["mask"], c["um"]) == t


def test_cube_cases(background_maps):
    cases = {c["name"]: c for c in THICKNESS}
    for name, c in cases.items():
        if name == "noise_three_trips":
            continue
        m = c["mask"]
        assert m.shape[1:] == (64, 64)  # one word per row: word = z * 64 + y
        # background on all six sides of every cube, inside the frame
        assert not (m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any())
    x, y, z = tc.CUBE_CENTRE
    for name, n in (("tie_two_trips", 2), ("tie_three_trips", 3)):
        c = cases[name]
        g = background_maps[name]
        zs, ys, xs = np.nonzero(c["mask"].astype(bool) & (g == 16_000_000))
        # the maximum exactly once per trip, in the same lane of the same workgroup
        assert list(zip(xs.tolist(), ys.tolist(), zs.tolist())) == [(x, y, z + tc.CUBE_PITCH * i) for i in range(n)]
        w0 = z * 64 + y
        assert [(zz * 64 + yy) for zz, yy in zip(zs.tolist(), ys.tolist())] == [w0 + tc.DIST_WORDS_PER_TRIP * i for i in range(n)]
    for name, sides in (("rising", (3, 5, 7)), ("falling", (7, 5, 3))):
        g = background_maps[name]
        got = [int(g[z + tc.CUBE_PITCH * i, y, x]) for i in range(3)]
        assert got == [((s + 1) // 2 * 1000) ** 2 for s in sides]  # one block per trip, each with its own maximum
        per_trip = [int(g[64 * i:64 * (i + 1)][cases[name]["mask"][64 * i:64 * (i + 1)].astype(bool)].max()) for i in range(2)]
        assert per_trip == got[:2]
    c = cases["winner_in_second_trip"]
    g = background_maps[c["name"]]
    first_trip = c["mask"][:64].astype(bool)
    assert first_trip.any() and int(g[:64][first_trip].max()) == (2 * 391) ** 2 < c["want"]["inscribed_um2"]
    c = cases["noise_three_trips"]
    assert c["mask"].shape[2] == 130 and int((background_maps[c["name"]][c["mask"].astype(bool)] == c["want"]["inscribed_um2"]).sum()) == 1


def test_view_case_sizes():
    d, h, w = tc.INIT_SHAPE
    wpr = (w + 63) // 64
    assert VIEWS["bright_full"]["raw"].shape == VIEWS["dark_sparse"]["raw"].shape == tc.INIT_SHAPE
    n = tc.projection_elements(tc.INIT_SHAPE)
    assert n == 279_760 and tc.trips(n, tc.VV_INIT_ELEMENTS_PER_TRIP) == 2
    # the z-projection (w * h elements, the first of the scratch) ends in the second trip: the y- and x-projections lie in it
    assert w * h > tc.VV_INIT_ELEMENTS_PER_TRIP
    # 128 columns x 16 rows x 8 planes per projection workgroup: more than one along every axis, so all atomics
    assert ((w + 127) // 128, (h + 15) // 16, (d + 7) // 8) == (5, 33, 2)
    assert h * wpr == 4680 and tc.trips(h * wpr, tc.VV_THREADS) == 19  # the point kernel over the z-shadow, the count kernel
    assert w % 64 == 8
    b = VIEWS["bright_full"]
    assert (b["raw"] == 4095).all() and b["mask"].all()
    s = VIEWS["dark_sparse"]
    assert int(s["raw"].max()) < 100 and s["raw"].min() != s["raw"].max()
    box = np.zeros(tc.INIT_SHAPE, np.uint8)
    box[2:7, 300:500, 330:515] = 1
    assert np.array_equal(s["mask"], box)
    # all three shadows and the sample projections of the sparse case differ from the bright one's nearly everywhere
    assert not s["mask"].any(axis=0).all() and not s["mask"].any(axis=1).all() and not s["mask"].any(axis=2).all()
    d, h, w = tc.DEEP_SHAPE
    wpr = (w + 63) // 64
    c = VIEWS["deep_point"]
    assert c["raw"].shape == tc.DEEP_SHAPE and d * wpr == 360 and tc.trips(d * wpr, tc.VV_THREADS) == 2
    zs, ys, xs = np.nonzero(c["mask"])
    assert (int(zs.min()), int(zs.max())) == (31, 37) and zs.min() * wpr >= tc.VV_THREADS  # z >= 29: the second trip
    assert 29 * wpr >= tc.VV_THREADS > 28 * wpr and int(zs.min()) >= 29  # plane 29 is the first one wholly in the second trip
    assert (int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())) == (3, 14, 400, 514)
    assert int(c["raw"].max()) > 4000
    for c in VIEWS.values():
        assert c["raw"].size <= 9 * 520 * 520 and c["why"]


@pytest.mark.parametrize("name", list(VIEWS))
def test_view_golden_equals_reference(native, name):
    from nm03_capstone_project_amd.ops import reference
    c = VIEWS[name]
    g = native.golden_volume_views(c["raw"], c["mask"], c["at"], c["type"], c["stored_bits"], c["inverted"])
    vc.assert_views_equal(g, reference.volume_views(c["raw"], c["mask"], c["at"], c["type"], c["stored_bits"], c["inverted"]))
    if name == "deep_point":
        assert list(g["mask_bbox"]) == [400, 3, 31, 514, 14, 37] and tuple(g["at"]) == (457, 8, 34)


def past_width_masks():
    out = [dc.case(n)["mask"] for n in tc.PAST_WIDTH_DISTANCE] + [mc.case(n)["mask"] for n in tc.PAST_WIDTH_MESH]
    by_id = {c["id"]: c for c in vc.all_cases()}
    return out + [by_id[n]["mask"] for n in tc.PAST_WIDTH_VIEWS] + [VIEWS["dark_sparse"]["mask"]]


def test_with_bits_past_width():
    import torch
    from nm03_capstone_project_amd import ops
    masks = past_width_masks()
    assert sorted({m.shape[2] for m in masks}) == [63, 65, 67, 70, 127, 129, 130, 520]
    for m in masks + [np.ones((2, 3, 128), np.uint8)]:
        d, h, w = m.shape
        t = torch.from_numpy(np.array(m)).bool()
        clean = ops.pack_bits(t)
        for words in (clean, clean.numpy()):  # a tensor and an array
            junk = tc.with_bits_past_width(words, w)
            assert junk.shape == words.shape and junk.dtype == words.dtype and junk is not words
            jt = torch.as_tensor(junk)
            assert torch.equal(ops.unpack_bits(jt, w), t)
            assert torch.equal(jt[..., :-1], clean[..., :-1])
            extra = (jt[..., -1] ^ clean[..., -1]).numpy().view(np.uint64)
            r = w % 64
            if r:
                assert (extra == np.uint64((2 ** 64 - 1) ^ ((1 << r) - 1))).all()  # every bit past the width, in every row
            else:
                assert not extra.any()
        assert torch.equal(ops.pack_bits(t), clean)  # the input is left alone
