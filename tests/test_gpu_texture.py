"""--measure-texture on the MI355X: the K12 kernels (k12_texture.hip) against the golden model and the NumPy
reference, matrices and integers compared with `==`."""
import os

import numpy as np
import pytest
import torch

from nm03_capstone_project_amd import ops
from nm03_capstone_project_amd.ops import reference

import texture_cases as tc
from conftest import run_bin

pytestmark = pytest.mark.gpu

CASES_2D = tc.cases_2d()
CASES_3D = tc.cases_3d()


def _dev(mask, raw):
    return torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(raw.view(np.int16)).cuda()


@pytest.fixture(scope="module")
def golden_2d(native):
    """The golden records of the 2D cases, computed once."""
    return {c[0]: native.golden_measure_texture(c[1], c[2], c[5], c[3], c[4]) for c in CASES_2D}


def test_every_2d_case_in_one_launch(native, golden_2d):
    """Every case in ONE batched launch of mixed sizes, sample formats and level counts, a workgroup per mask."""
    dev = [_dev(c[1], c[2]) for c in CASES_2D]
    args = ([d[0] for d in dev], [d[1] for d in dev], [c[5] for c in CASES_2D], [c[3] for c in CASES_2D], [c[4] for c in CASES_2D])
    got = ops.measure_texture(*args)
    assert len(got) == len(CASES_2D)
    for (name, mask, raw, ptype, bits, levels), rec in zip(CASES_2D, got):
        assert tc.same(rec, golden_2d[name]), name
    hom = got[[c[0] for c in CASES_2D].index("full_512_homogeneous")]["glcm"]
    assert hom[0, 0] == tc.HOMOGENEOUS_512_CELL and np.count_nonzero(hom) == 1
    har = got[[c[0] for c in CASES_2D].index("haralick_4x4")]
    assert (har["glcm"] == tc.HARALICK_MERGED).all() and har["pairs"] == 42
    # the same launch again: nothing is left behind in the records
    again = ops.measure_texture(*args)
    assert all(tc.same(a, b) for a, b in zip(again, got))


def test_2d_tensor_batch_and_single_slice(native):
    r = np.random.default_rng(71)
    mask = r.random((3, 33, 129)) < 0.6
    raw = r.integers(0, 65536, size=mask.shape).astype(np.uint16)
    m, x = _dev(mask, raw)
    got = ops.measure_texture(m, x, 16)
    for i in range(3):
        assert tc.same(got[i], reference.glcm(mask[i], raw[i], 16))
    assert tc.same(ops.measure_texture(m[1], x[1], 16)[0], got[1])


def test_stray_plane_bits_past_the_width_do_not_pair(native, golden_2d):
    """The bit planes as a kernel may find them: every storage bit past the width set."""
    names = ("70x5", "65x2", "checkerboard")
    planes, samples, hs, ws, lv, types, bits = [], [], [], [], [], [], []
    for name in names:
        _, mask, raw, ptype, b, levels = next(c for c in CASES_2D if c[0] == name)
        m, x = _dev(mask, raw)
        h, w = mask.shape
        p = ops.pack_bits(m.unsqueeze(0)).reshape(h, -1).clone()
        p[:, -1] |= -1 << (w & 63)
        planes.append(p.reshape(-1))
        samples.append(x.reshape(-1))
        hs.append(h), ws.append(w), lv.append(levels), types.append(ptype), bits.append(b)
    pl, sm = torch.cat(planes).contiguous(), torch.cat(samples).contiguous()
    got = native.k_measure_texture(pl.data_ptr(), sm.data_ptr(), hs, ws, lv, types, bits, torch.cuda.current_stream().cuda_stream)
    for name, rec in zip(names, got):
        assert tc.same(rec, golden_2d[name]), name


@pytest.mark.parametrize("name,mask,raw,ptype,bits,levels", CASES_3D, ids=tc.ids(CASES_3D))
def test_measure_volume_texture_equals_golden(native, name, mask, raw, ptype, bits, levels):
    m, x = _dev(mask, raw)
    got = ops.measure_volume_texture(m, x, levels, ptype, bits)
    assert tc.same(got, native.golden_measure_volume_texture(mask, raw, levels, ptype, bits))
    assert tc.same(got, ops.measure_volume_texture(m, x, levels, ptype, bits))  # the accumulators are reset by the first launch


def test_2d_and_3d_agree_on_one_plane(native, golden_2d):
    _, mask, raw, ptype, bits, levels = next(c for c in CASES_2D if c[0] == "256x300")
    m, x = _dev(mask, raw)
    assert tc.same(ops.measure_volume_texture(m.unsqueeze(0), x.unsqueeze(0), levels, ptype, bits), golden_2d["256x300"])


def test_ops_reject_bad_arguments():
    m = torch.zeros((3, 4), dtype=torch.bool, device="cuda")
    raw = torch.zeros((3, 4), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw[:2])
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw.float())
    with pytest.raises(ValueError):
        ops.measure_texture(m.cpu(), raw)
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw, stored_bits=17)
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw, levels=65)
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw, levels=1)
    with pytest.raises(ValueError):
        ops.measure_texture([], [])
    with pytest.raises(ValueError):
        ops.measure_texture([m, m], [raw, raw], [8])  # one entry per slice
    with pytest.raises(ValueError):
        ops.measure_texture(m, raw, pixel_type="f32")
    with pytest.raises(ValueError):
        ops.measure_volume_texture(m, raw)
    with pytest.raises(ValueError):
        ops.measure_volume_texture(m.unsqueeze(0), raw.unsqueeze(0), levels=0)
    rec = ops.measure_volume_texture(m.unsqueeze(0), raw.unsqueeze(0))
    assert rec["samples"] == 0 and rec["pairs"] == 0 and not rec["glcm"].any()


# ---------------------------------------------------------------------------------------------
# SlicePipeline / run_array
# ---------------------------------------------------------------------------------------------
def _slices(native):
    return [native.phantom_slice(256, 256, p, s, 25, 7) for p, s in ((3, 12), (1, 10))]


META = {"type": "u16", "stored_bits": 16, "slope": 2.0, "intercept": -100.0, "spacing_x": 0.5, "spacing_y": 0.75}


def test_run_array_with_the_flag_equals_golden(native):
    import nm03_capstone_project_amd as nm
    on = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure_texture=True))
    on63 = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure_texture=True, texture_levels=63))
    some = 0
    for raw in _slices(native):
        raw = np.ascontiguousarray(raw, dtype=np.uint16)
        for pipe, levels in ((on, 32), (on63, 63)):
            r, g = pipe.run_array(raw, META), pipe.golden(raw, META)
            assert tc.same(r["texture"], g["texture"]) and r["measure_json"] == g["measure_json"] and r["measure"] == g["measure"]
            assert tc.same(r["texture"], reference.glcm(r["dilated"], raw, levels))
            assert r["texture"]["samples"] == r["measure"]["area_px"]
            some += r["texture"]["pairs"] > 0
    assert some == 4, "masks without pairs prove nothing"


def test_every_flag_together_leaves_the_other_outputs_alone(native):
    """measure, measure_diameters, measure_intensity and measure_texture in one engine: everything but the
    texture record and the appended keys equals the run without the texture flag."""
    import nm03_capstone_project_amd as nm
    kw = dict(batch_size=2, streams=1, measure=True, measure_diameters=True, measure_intensity=True)
    allf = nm.SlicePipeline(nm.PipelineConfig(measure_texture=True, **kw))
    rest = nm.SlicePipeline(nm.PipelineConfig(**kw))
    for raw in _slices(native):
        raw = np.ascontiguousarray(raw, dtype=np.uint16)
        a, b = allf.run_array(raw, META), rest.run_array(raw, META)
        assert "texture" in a and "texture" not in b
        assert set(a) - {"texture"} == set(b)
        for k in b:
            if k == "measure_json":
                assert a[k] == b[k][:-2] + native.texture_keys(a["texture"]["glcm"]) + "}\n"
            elif isinstance(b[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k
            elif isinstance(b[k], (bytes, dict, str, int)):
                assert a[k] == b[k], k
        assert a["measure_json"] == allf.golden(raw, META)["measure_json"]


def test_an_engine_without_the_flag_is_unchanged(native):
    """Built without the flag the engine launches nothing new: its keys, records and text are today's."""
    import nm03_capstone_project_amd as nm
    off = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure=True))
    for raw in _slices(native):
        raw = np.ascontiguousarray(raw, dtype=np.uint16)
        r, g = off.run_array(raw, META), off.golden(raw, META)
        assert "texture" not in r and "texture" not in g
        assert r["measure_json"] == g["measure_json"] and "glcm" not in r["measure_json"] and r["measure"] == g["measure"]
        assert r["measure"] == native.golden_measure(r["dilated"].astype(np.uint8), r["region"].astype(np.uint8), raw, "u16", 16, 8)


# ---------------------------------------------------------------------------------------------
# VolumePipeline(measure=True, measure_texture=True)
# ---------------------------------------------------------------------------------------------
def test_volume_pipeline_equals_golden_measure(native):
    import nm03_capstone_project_amd as nm
    import volume_cases as vc
    vol = vc.serpentine_volume(**vc.SERPENTINE)
    kw = dict(spacing=(0.5, 0.75, 2.5), spacing_z_source="spacing_between_slices")
    vp = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_texture=True, texture_levels=24)
    res = vp.run(vol, **kw)
    rec, text, texture = vp.golden_measure(res["dilated"], res["region"], vol, **kw)
    assert tc.same(res["texture"], texture) and res["measure_json"] == text and res["measure"] == rec
    assert tc.same(texture, reference.glcm(res["dilated"], vol, 24)) and texture["samples"] == rec["volume_vox"] > 0
    assert texture["pairs"] > 0
    off = nm.VolumePipeline(connectivity=6, dilation=7, measure=True)
    res0 = off.run(vol, **kw)
    assert "texture" not in res0 and res0["measure_json"] == off.golden_measure(res["dilated"], res["region"], vol, **kw)[1]
    assert text.startswith(res0["measure_json"][:-2] + ',"glcm_levels":24,')
    va = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_lesions=2, measure_intensity=True,
                           measure_texture=True, texture_levels=24)
    resa = va.run(vol, **kw)
    reca, texta, lesions, intensity, texa = va.golden_measure(resa["dilated"], resa["region"], vol, **kw)
    assert (resa["measure"], resa["measure_json"], resa["lesions"], resa["intensity"]) == (reca, texta, lesions, intensity)
    assert tc.same(resa["texture"], texa) and tc.same(texa, texture)


def test_run_slab_refuses_texture(native):
    vol = np.zeros((4, 16, 64), np.uint16)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError, match="slabs"):
        runner.run_slab(native.self_comm(), vol, 0, 4, native.PipelineParams(), 6, 3, [], measure_texture=True)
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure_texture=True)  # needs measure
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure=True, measure_texture=True, texture_levels=65)


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


@pytest.fixture(scope="module")
def two_patients(tmp_path_factory, native):
    root = str(tmp_path_factory.mktemp("gtdata")) + "/"
    native.synth_cohort(root, patients=2, min_slices=3, max_slices=3, threads=2)
    return root


def _cli(data, out, *args):
    r = run_bin("img_processing_parallel", "--quiet", *args, "--data-root", data, "--out", str(out))
    assert r.returncode == 0, r.stderr
    return tree(out)


def test_cli_2d_gpu_equals_cpu(two_patients, tmp_path):
    flags = ("--measure-texture", "--measure-intensity", "--measure-diameters")
    cpu = _cli(two_patients, tmp_path / "cpu", "--cpu", *flags)
    gpu = _cli(two_patients, tmp_path / "gpu", *flags)
    names = [k for k in gpu if k.endswith("_measure.json")]
    assert len(names) == 6 and "measurements.csv" in gpu
    assert all(gpu[k] == cpu[k] for k in names) and gpu["measurements.csv"] == cpu["measurements.csv"]
    assert set(gpu) == set(cpu) and b'"glcm_contrast":' in gpu[names[0]]


def test_cli_3d_gpu_equals_cpu(two_patients, tmp_path):
    flags = ("--mode", "3d", "--measure-texture", "--texture-levels", "64", "--measure-intensity")
    cpu = _cli(two_patients, tmp_path / "cpu", "--cpu", *flags)
    gpu = _cli(two_patients, tmp_path / "gpu", *flags)
    names = [k for k in gpu if k.endswith("volume_measure.json")]
    assert len(names) == 2 and all(gpu[k] == cpu[k] for k in names) and gpu["volumes.csv"] == cpu["volumes.csv"]
    assert b'"glcm_levels":64,' in gpu[names[0]] and set(gpu) == set(cpu)
