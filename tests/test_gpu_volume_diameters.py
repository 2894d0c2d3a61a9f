"""Per-lesion 3D and axial diameters on the MI355X: the K13 kernels (k13_volume_diameters.hip, after K10 between
K8's two passes) against the golden model, with the tile skipping on and off; repeated calls, a smaller
volume on the table a larger one left behind, and the unflagged op unchanged."""
import functools

import numpy as np
import pytest
import torch

from nm03_capstone_project_amd import ops

import volume_diameter_cases as vdc
import volume_lesion_cases as vlc

pytestmark = pytest.mark.gpu

GPU_CASES = vdc.gpu_cases()


@functools.lru_cache(maxsize=None)
def _mask(name):
    return next(build for cid, build, _ in GPU_CASES if cid == name)()


def _dev(mask):
    return torch.from_numpy(mask.astype(bool)).cuda()


@pytest.mark.parametrize("conn", vdc.CONNS)
@pytest.mark.parametrize("name,n", [(c[0], c[2]) for c in GPU_CASES], ids=[c[0] for c in GPU_CASES])
def test_measure_volume_diameters_equals_golden(native, name, n, conn):
    mask = _mask(name)
    t = _dev(mask)
    for um in vdc.SPACINGS:
        golden = native.golden_measure_volume_diameters(mask, n, um, conn)
        assert ops.measure_volume_diameters(t, n, um, conn) == golden, um
        assert ops.measure_volume_diameters(t, n, um, conn, brute_force=True) == golden, um


def test_hand_worked_example_on_the_gpu(native):
    assert ops.measure_volume_diameters(_dev(vdc.hand_box()), 1) == [vdc.HAND]


def test_repeated_calls_and_a_smaller_volume_on_a_stale_table(native):
    """Twice on the same tensor (no dependence on the order of the atomics or of the workgroups), then a
    small volume on the work buffer the large one left behind, then the large one again at another N."""
    big, small = vdc.ellipsoid(), vlc.word_straddle(65)
    tb, ts = _dev(big), _dev(small)
    um = (977, 1020, 3300)
    first = ops.measure_volume_diameters(tb, 2, um, 26)
    assert first == ops.measure_volume_diameters(tb, 2, um, 26)
    assert first == native.golden_measure_volume_diameters(big, 2, um, 26)
    assert ops.measure_volume_diameters(ts, 3, um, 6) == native.golden_measure_volume_diameters(small, 3, um, 6)
    assert ops.measure_volume_diameters(tb, 64, um, 26) == first
    assert ops.measure_volume_diameters(ts, 1, um, 6) == native.golden_measure_volume_diameters(small, 1, um, 6)


def test_lesions_op_unchanged_next_to_the_diameters(native):
    """ops.measure_volume_lesions before and after a diameter call: the same records, equal to golden."""
    mask = vdc.combs()
    region, raw = vlc.inputs(mask)
    t = (torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(region.astype(bool)).cuda(),
         torch.from_numpy(raw.view(np.int16)).cuda())
    before = ops.measure_volume_lesions(*t, 2, 26)
    dia = ops.measure_volume_diameters(t[0], 2, (1000, 1000, 1000), 26)
    assert ops.measure_volume_lesions(*t, 2, 26) == before
    assert before[1] == native.golden_measure_volume_lesions(mask, raw, 2, "u16", 16, 26)
    assert before[0] == native.golden_measure_volume(mask, region, raw, "u16", 16, 26)
    # the rows both combs share are attributed to the right one
    assert [d["major"] for d in dia] == [d["major"] for d in native.golden_measure_volume_diameters(mask, 2, (1000, 1000, 1000), 26)]


def test_refusals_on_the_gpu(native):
    t = _dev(np.ones((2, 2, 3), np.uint8))
    with pytest.raises(ValueError, match=r"\(w - 1\) \* ux = 2 \* 1073741824"):
        ops.measure_volume_diameters(t, 1, (2 ** 30, 1000, 1000))
    with pytest.raises(ValueError):
        ops.measure_volume_diameters(t, 0)
    with pytest.raises(ValueError):
        ops.measure_volume_diameters(t, 1, (1000, 0, 1000))
    with pytest.raises(ValueError):
        ops.measure_volume_diameters(t.cpu(), 1)
    assert len(ops.measure_volume_diameters(t, 1, (2 ** 30 - 1, 2 ** 31 - 1, 2 ** 31 - 1))) == 1


@pytest.mark.parametrize("conn", vdc.CONNS)
def test_the_largest_admissible_spacings_on_the_ellipsoid(native, conn):
    """vdc.ELLIPSOID_MAX_UM: squared distances above 2^61 and tile bounds towards 3 · 2^62, which only
    unsigned 64-bit integers order right. Equal to golden with the tile skipping on and off,
    and consistent in Python integers."""
    mask, um = vdc.ellipsoid(), vdc.ELLIPSOID_MAX_UM
    t = _dev(mask)
    golden = native.golden_measure_volume_diameters(mask, 2, um, conn)
    assert len(golden) == 1 and golden[0]["major_um2"] > 2 ** 61
    for brute in (False, True):
        got = ops.measure_volume_diameters(t, 2, um, conn, brute_force=brute)
        assert got == golden, brute
        assert all(vdc.pair_holds(d, um) for d in got)


# ---------------------------------------------------------------------------------------------
# VolumePipeline(measure=True, measure_lesions=N, measure_diameters=True)
# ---------------------------------------------------------------------------------------------
def test_pipeline_measures_the_diameters_of_the_serpentine(native):
    import nm03_capstone_project_amd as nm
    import volume_cases as vc
    strip_new_keys = vdc.strip_new_keys
    vol = vc.serpentine_volume(**vc.SERPENTINE)
    spacing = (0.5, 0.75, 2.5)
    vp = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_lesions=4, measure_diameters=True)
    res = vp.run(vol, spacing=spacing, spacing_z_source="spacing_between_slices")
    rec, text, lesions, dia = vp.golden_measure(res["dilated"], res["region"], vol, spacing=spacing,
                                                spacing_z_source="spacing_between_slices")
    assert res["diameters"] == dia and res["measure_json"] == text and res["lesions"] == lesions and res["measure"] == rec
    assert dia and all(vdc.pair_holds(d, (500, 750, 2500)) for d in dia)
    # without the flag: the same run, and the text is this one with the new keys taken out
    without = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_lesions=4)
    res0 = without.run(vol, spacing=spacing, spacing_z_source="spacing_between_slices")
    assert "diameters" not in res0 and res0["measure_json"] == strip_new_keys(text) and res0["lesions"] == lesions
    for k in ("band", "region", "dilated"):
        assert np.array_equal(res0[k], res[k]), k
    # the same runner: more lesions (the row table regrows), then a smaller volume (buffers rebuilt)
    vp.measure_lesions = 9
    res9 = vp.run(vol, spacing=spacing)
    assert res9["diameters"] == vp.golden_measure(res9["dilated"], res9["region"], vol, spacing=spacing)[3]
    assert res9["diameters"][:len(dia)] == dia
    small = vol[:24, :60]
    vp.measure_lesions = 2
    res2 = vp.run(small)
    assert res2["diameters"] == vp.golden_measure(res2["dilated"], res2["region"], small)[3]


def test_runner_refusals(native):
    vol = np.zeros((4, 16, 64), np.uint16)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError, match="slabs"):
        runner.run_slab(native.self_comm(), vol, 0, 4, native.PipelineParams(), 6, 3, [], measure_diameters=True)
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure=True, measure_diameters=True)  # needs lesions
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure_diameters=True)  # needs measure
    with pytest.raises(ValueError, match=r"\(w - 1\) \* ux"):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure=True, measure_lesions=1, measure_diameters=True,
                   spacing=[40000.0, 1.0, 1.0])  # 63 · 40 000 000 um ≥ 2^31


# ---------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------
def test_cli_gpu_equals_cpu_and_unflagged_tree_unchanged(cohort_root, tmp_path):
    from conftest import run_bin
    strip_new_keys, tree = vdc.strip_new_keys, vdc.tree

    def cli(out, *args):
        r = run_bin("img_processing_parallel", "--mode", "3d", "--quiet", *args, "--data-root", cohort_root, "--out", str(out))
        assert r.returncode == 0, r.stderr
        return tree(out)

    flags = ("--measure-volume-lesions", "3", "--measure-volume-diameters")
    cpu = cli(tmp_path / "cpu", "--cpu", *flags)
    gpu = cli(tmp_path / "gpu", *flags)
    assert "lesions.csv" in gpu and sum(k.endswith("volume_measure.json") for k in gpu) == 4
    assert gpu == cpu
    # without the flag: the tree K10 alone writes, on the GPU as on the CPU
    les = cli(tmp_path / "les", "--measure-volume-lesions", "3")
    assert les == cli(tmp_path / "lescpu", "--cpu", "--measure-volume-lesions", "3")
    assert set(les) == set(gpu)
    for k in les:
        if k.endswith("volume_measure.json"):
            assert strip_new_keys(gpu[k].decode()).encode() == les[k]
        elif k != "lesions.csv":
            assert gpu[k] == les[k], k
