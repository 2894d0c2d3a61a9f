"""--measure-volume-lesions on the MI355X: the K10 kernels (k10_volume_lesions.hip, between K8's two passes)
against the golden model; the pipeline, the slab refusal and the CLI."""
import functools
import os

import numpy as np
import pytest
import torch

import nm03_capstone_project_amd as nm
from nm03_capstone_project_amd import ops

import volume_cases as vc
import volume_lesion_cases as vlc
import volume_measure_cases as vmc
from conftest import run_bin

pytestmark = pytest.mark.gpu

GPU_CASES = vlc.gpu_cases()


def _dev(mask, region, raw):
    return (torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(region.astype(bool)).cuda(),
            torch.from_numpy(raw.view(np.int16)).cuda())


@pytest.mark.parametrize("conn", vlc.CONNS)
@pytest.mark.parametrize("name,build", GPU_CASES, ids=[c[0] for c in GPU_CASES])
def test_measure_volume_lesions_equals_golden(native, name, build, conn):
    mask = build()
    region, raw = vlc.inputs(mask)
    t = _dev(mask, region, raw)
    plain = ops.measure_volume(*t, conn)
    assert plain == native.golden_measure_volume(mask, region, raw, "u16", 16, conn)
    for n in vlc.LESION_COUNTS:
        rec, lesions = ops.measure_volume_lesions(*t, n, conn)
        assert lesions == native.golden_measure_volume_lesions(mask, raw, n, "u16", 16, conn), n
        assert rec == plain, n  # the cavity pass after the lesion phase still sees its scratch


@pytest.mark.parametrize("ptype,bits", [("i16", 16), ("u16", 12)])
def test_measure_volume_lesions_sample_formats(native, ptype, bits):
    mask = vmc.noise(vmc.NOISE_SHAPE, 0.31)
    raw = vmc.raw_for(mask.shape, seed=bits)
    rec, lesions = ops.measure_volume_lesions(*_dev(mask, mask, raw), 64, 6, ptype, bits)
    assert lesions == native.golden_measure_volume_lesions(mask, raw, 64, ptype, bits, 6)
    assert rec == native.golden_measure_volume(mask, mask, raw, ptype, bits, 6)


@functools.lru_cache(maxsize=None)
def _cohort_sized():
    mask = vmc.noise(vmc.COHORT_SHAPE, 0.31)
    return mask, vmc.region_for(mask), vmc.raw_for(mask.shape)


def test_cohort_sized_noise_repeatable_and_scratch_reuse(native):
    """25 × 256 × 256 at density 0.31, 6-connected, near the percolation threshold: a broad spread of
    component sizes over 1600 workgroups, many more components than records, and a giant lesion with
    stretches in most workgroups. Twice on the same tensors (no dependence on the order of the appends or
    of the atomics), then a smaller volume on the scratch the large one left behind."""
    mask, region, raw = _cohort_sized()
    t = _dev(mask, region, raw)
    first = ops.measure_volume_lesions(*t, 64, 6)
    assert first == ops.measure_volume_lesions(*t, 64, 6)
    golden = native.golden_measure_volume_lesions(mask, raw, 64, "u16", 16, 6)
    assert first[1] == golden and len(golden) == 64 and first[0]["components"] > 64
    assert first[0] == ops.measure_volume(*t, 6)
    small = vlc.word_straddle(65)
    sregion, sraw = vlc.inputs(small)
    rec, lesions = ops.measure_volume_lesions(*_dev(small, sregion, sraw), 3, 6)
    assert lesions == native.golden_measure_volume_lesions(small, sraw, 3, "u16", 16, 6) and len(lesions) == 2
    assert rec == native.golden_measure_volume(small, sregion, sraw, "u16", 16, 6)


def test_measure_volume_lesions_rejects_bad_arguments():
    m = torch.zeros((2, 3, 4), dtype=torch.bool, device="cuda")
    raw = torch.zeros((2, 3, 4), dtype=torch.int16, device="cuda")
    for n in (0, 65):
        with pytest.raises(ValueError):
            ops.measure_volume_lesions(m, m, raw, n)
    with pytest.raises(ValueError):
        ops.measure_volume_lesions(m, m, raw, 3, connectivity=18)
    with pytest.raises(ValueError):
        ops.measure_volume_lesions(m, m[:1], raw, 3)
    assert ops.measure_volume_lesions(m, m, raw, 3)[1] == []


# ---------------------------------------------------------------------------------------------
# VolumePipeline(measure=True, measure_lesions=N)
# ---------------------------------------------------------------------------------------------
def test_pipeline_measures_the_lesions_of_the_serpentine(native):
    vol = vc.serpentine_volume(**vc.SERPENTINE)
    spacing = (0.5, 0.75, 2.5)
    vp = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_lesions=4)
    res = vp.run(vol, spacing=spacing, spacing_z_source="spacing_between_slices")
    rec, text, lesions = vp.golden_measure(res["dilated"], res["region"], vol, spacing=spacing,
                                           spacing_z_source="spacing_between_slices")
    assert res["lesions"] == lesions and res["measure_json"] == text and res["measure"] == rec
    assert lesions and lesions[0]["voxels"] == rec["largest_vox"]
    plain = nm.VolumePipeline(connectivity=6, dilation=7).run(vol)
    for k in ("band", "region", "dilated"):
        assert np.array_equal(plain[k], res[k]), k
    without = nm.VolumePipeline(connectivity=6, dilation=7, measure=True)
    res0 = without.run(vol, spacing=spacing, spacing_z_source="spacing_between_slices")
    assert "lesions" not in res0
    assert res0["measure_json"] == without.golden_measure(res["dilated"], res["region"], vol, spacing=spacing,
                                                          spacing_z_source="spacing_between_slices")[1]
    assert text.startswith(res0["measure_json"][:-2] + ",\"lesions_max\":4,")
    # The same runner, another N and a smaller volume (buffers rebuilt for the new shape).
    small = vol[:24, :60]
    vp.measure_lesions = 2
    res2 = vp.run(small)
    assert res2["lesions"] == vp.golden_measure(res2["dilated"], res2["region"], small)[2]


def test_run_slab_refuses_lesions(native):
    vol = np.zeros((4, 16, 64), np.uint16)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError, match="slabs"):
        runner.run_slab(native.self_comm(), vol, 0, 4, native.PipelineParams(), 6, 3, [], measure_lesions=3)
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure_lesions=3)  # needs measure
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure=True, measure_lesions=65)


# ---------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------
def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _cli(cohort_root, out, *args, env=None):
    r = run_bin("img_processing_parallel", "--mode", "3d", "--quiet", *args, "--data-root", cohort_root, "--out", str(out),
                env=env)
    assert r.returncode == 0, r.stderr
    return tree(out)


def test_cli_gpu_equals_cpu_and_two_ranks(cohort_root, tmp_path):
    cpu = _cli(cohort_root, tmp_path / "cpu", "--cpu", "--measure-volume-lesions", "3")
    gpu = _cli(cohort_root, tmp_path / "gpu", "--measure-volume-lesions", "3")
    assert "lesions.csv" in gpu and "volumes.csv" in gpu and sum(k.endswith("volume_measure.json") for k in gpu) == 4
    assert gpu == cpu
    two = _cli(cohort_root, tmp_path / "two", "--measure-volume-lesions", "3", "--gpus", "2", env={"NM03_DEVICE_OVERRIDE": "0"})
    assert two == gpu
    vol = _cli(cohort_root, tmp_path / "vol", "--measure-volume")
    assert set(gpu) - set(vol) == {"lesions.csv"}
    assert all(gpu[k] == vol[k] for k in vol if not k.endswith("volume_measure.json"))
    assert all(gpu[k].startswith(vol[k][:-2] + b",\"lesions_max\":3,") for k in vol if k.endswith("volume_measure.json"))
