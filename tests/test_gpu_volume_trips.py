"""K14, K15 and K16 on the GPU where their strided loops take more than one trip and where the mask words carry bits past
the width, against the golden model, everything compared with ==. The inputs are volume_trip_cases (their properties
are asserted on the CPU by test_volume_trip_cases.py). What each test runs that no other test does:
  test_thickness_strides_past_the_slots      vdist_planes_kernel<thickness> on more than 4096 words: a workgroup's
                                             second and third trip, a tie between two trips of one lane, a winner found
                                             in a later trip and one that has to survive later trips
  test_views_after_a_brighter_volume         vv_init_kernel's second trip: every element of the reused scratch holds 4095
                                             or a set bit when a dark, sparse volume of the same shape follows; 19 trips
                                             of the point and the count kernel
  test_views_point_found_on_a_later_trip     vv_point_kernel's z loop with both extremes in its second trip
  test_kernels_ignore_bits_past_the_width    the K14, K15 and K16 kernels on words whose storage bits past the width are
                                             set (the ops only ever pack clean words); the margin writes them as 0
  test_runner_thickness_on_a_deep_volume     the thickness loop's second trip on VolumeRunner's own buffers (20 planes,
                                             6240 words), after the margin, with measure, views and mesh of that mask"""
import json

import numpy as np
import pytest

import volume_distance_cases as dc
import volume_export_cases as xc
import volume_mesh_cases as mc
import volume_trip_cases as tc
import volume_view_cases as vc

pytestmark = pytest.mark.gpu

THICKNESS = tc.thickness_cases()
VIEWS = tc.view_cases()


def on_gpu(a):
    import torch
    a = np.array(a)  # a writable copy
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def golden_views(native, c):
    return native.golden_volume_views(c["raw"], c["mask"], c["at"], c["type"], c["stored_bits"], c["inverted"])


@pytest.mark.parametrize("c", THICKNESS, ids=dc.ids(THICKNESS))
def test_thickness_strides_past_the_slots(native, c):
    import torch
    import nm03_capstone_project_amd as nm
    assert tc.word_count(c["mask"].shape) > tc.DIST_WORDS_PER_TRIP
    mask = on_gpu(c["mask"]).bool()
    um = list(c["um"])
    want = native.golden_volume_thickness(c["mask"], um)
    assert {k: want[k] for k in c["want"]} == c["want"]
    got = nm.ops.volume_thickness(mask, um)
    assert dc.thickness_equal(got, want) and got == want
    if c["name"] in tc.MAP_CASES:
        dist = nm.ops.volume_distance(mask, um, to="background")
        assert np.array_equal(dist.cpu().numpy(), native.golden_volume_distance(c["mask"], um, True, None))
    torch.cuda.synchronize()


def test_views_after_a_brighter_volume(native):
    import nm03_capstone_project_amd as nm
    bright, dark = VIEWS["bright_full"], VIEWS["dark_sparse"]
    inputs = {c["id"]: (on_gpu(c["raw"]), on_gpu(c["mask"]).bool()) for c in (bright, dark)}
    wants = {c["id"]: golden_views(native, c) for c in (bright, dark)}
    assert wants["dark_sparse"]["views"]["mip_axial"]["raw_max"] < 100 and wants["bright_full"]["views"]["mip_sagittal"]["raw_min"] == 4095
    for c in (bright, dark, bright):  # nothing in between: the op's scratch is the one the run before left
        raw, mask = inputs[c["id"]]
        got = nm.ops.volume_views(raw, mask, at=c["at"], pixel_type=c["type"], stored_bits=c["stored_bits"], inverted=c["inverted"])
        vc.assert_views_equal(got, wants[c["id"]])


def test_views_point_found_on_a_later_trip(native):
    import nm03_capstone_project_amd as nm
    c = VIEWS["deep_point"]
    want = golden_views(native, c)
    got = nm.ops.volume_views(on_gpu(c["raw"]), on_gpu(c["mask"]).bool(), at="mask")
    assert tuple(got["at"]) == tuple(want["at"]) == (457, 8, 34) and list(got["mask_bbox"]) == list(want["mask_bbox"]) == [400, 3, 31, 514, 14, 37]
    vc.assert_views_equal(got, want)


# ---- bits past the width: the kernels directly, on words no op would pass -------------------------------
def junk_words(mask):
    """The packed words of a [D, H, W] mask with every bit past the width set, on the GPU."""
    import torch
    import nm03_capstone_project_amd as nm
    w = mask.shape[2]
    assert w % 64 != 0
    clean = nm.ops.pack_bits(on_gpu(mask).bool()).contiguous()
    words = tc.with_bits_past_width(clean, w).contiguous()
    assert not torch.equal(words, clean) and torch.equal(nm.ops.unpack_bits(words, w), nm.ops.unpack_bits(clean, w))
    return words


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def distance_kernels_on_junk(native, name):
    import torch
    import nm03_capstone_project_amd as nm
    c = dc.case(name)
    d, h, w = c["mask"].shape
    um = list(c["um"])
    words = junk_words(c["mask"])
    for to in dc.POLARITIES:
        for cap in c["caps"]:
            out = torch.empty((d, h, w), dtype=torch.int64, device="cuda")
            native.k_volume_distance(words.data_ptr(), w, h, d, um, "map", to == "background", -1 if cap is None else cap, out.data_ptr(),
                                     stream())
            assert np.array_equal(out.cpu().numpy(), native.golden_volume_distance(c["mask"], um, to == "background", cap)), (to, cap)
    for r in (0, um[0], um[2], 2 * max(um) + 1):
        out = torch.full_like(words, -1)
        native.k_volume_distance(words.data_ptr(), w, h, d, um, "margin", False, r, out.data_ptr(), stream())
        want = nm.ops.pack_bits(torch.from_numpy(native.golden_dilate3d_mm(c["mask"], um, r)).bool())
        assert torch.equal(out.cpu(), want), r  # the raw words: the bits past the width come back 0
    got = native.k_volume_distance(words.data_ptr(), w, h, d, um, "thickness", True, -1, 0, stream())
    assert got == native.golden_volume_thickness(c["mask"], um)


def mesh_kernels_on_junk(native, name):
    c = mc.case(name)
    d, h, w = c["mask"].shape
    words = junk_words(c["mask"])
    for pl in mc.PLACEMENTS:
        got = native.k_volume_mesh(words.data_ptr(), w, h, d, [float(v) for v in c["spacing"]], pl, 0, 512 << 20, stream())
        mc.assert_mesh_equal(got, native.golden_volume_mesh(c["mask"], list(c["spacing"]), pl))


def views_kernels_on_junk(native, name):
    c = VIEWS[name] if name in VIEWS else next(x for x in vc.all_cases() if x["id"] == name)
    d, h, w = c["mask"].shape
    words = junk_words(c["mask"])
    raw = on_gpu(c["raw"]).contiguous()
    got = native.k_volume_views(raw.data_ptr(), words.data_ptr(), w, h, d, h * w, c["at"], c["type"], c["stored_bits"], c["inverted"],
                                stream())
    vc.assert_views_equal(got, golden_views(native, c))


PAST_WIDTH = ([("k16", n) for n in tc.PAST_WIDTH_DISTANCE] + [("k15", n) for n in tc.PAST_WIDTH_MESH] +
              [("k14", n) for n in tc.PAST_WIDTH_VIEWS + ("dark_sparse",)])


@pytest.mark.parametrize("kernel,name", PAST_WIDTH, ids=[f"{k}-{n}" for k, n in PAST_WIDTH])
def test_kernels_ignore_bits_past_the_width(native, kernel, name):
    {"k16": distance_kernels_on_junk, "k15": mesh_kernels_on_junk, "k14": views_kernels_on_junk}[kernel](native, name)


# ---- the runner ---------------------------------------------------------------------------------------
DEEP_VOL_SHAPE = (20, 104, 136)  # d, h, w: the phantom of test_gpu_volume_distance.py with 20 planes, 6240 words, two trips
VOL_SPACING = (0.5, 0.75, 5.0)
VOL_UM = [500, 750, 5000]


def test_runner_thickness_on_a_deep_volume(native):
    import nm03_capstone_project_amd as nm
    d, h, w = DEEP_VOL_SHAPE
    assert tc.trips(tc.word_count(DEEP_VOL_SHAPE), tc.DIST_WORDS_PER_TRIP) == 2
    s0 = xc.slice0(d)
    volume = np.stack([native.phantom_slice(h, w, 3, s0 + k, xc.NSLICES, xc.SEED) for k in range(d)]).astype(np.uint16)
    pipe = nm.VolumePipeline(nm.PipelineConfig(), dilate_mm=1.2, measure=True, measure_thickness=True, views=True, mesh=True)
    res = pipe.run(volume, spacing=VOL_SPACING)
    dil = native.golden_dilate3d_mm(res["region"], VOL_UM, 1200)
    assert res["region"].sum() > 0 and np.array_equal(res["dilated"], dil)
    rec, text, thickness = pipe.golden_measure(dil, res["region"], volume, spacing=VOL_SPACING)
    assert res["measure"] == rec and res["thickness"] == thickness
    assert res["measure_json"] == text and json.loads(text)["thickness_spacing_um"] == VOL_UM
    assert thickness == native.golden_volume_thickness(dil, VOL_UM) and thickness["found"]
    mc.assert_mesh_equal(res["mesh"], native.golden_volume_mesh(dil, list(VOL_SPACING), "corner"))
    gv = native.golden_volume_views(volume, dil, "mask")
    assert tuple(gv["at"]) == res["views_at"]
    for name, v in gv["views"].items():
        assert np.array_equal(res["views"][name]["mask"], v["mask"]) and np.array_equal(res["views"][name]["raw"], v["raw"]), name
        assert res["views"][name]["mask_px"] == v["mask_px"]
