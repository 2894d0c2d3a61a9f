"""--measure-intensity on the MI355X: the K11 kernels (k11_intensity.hip) against the golden model and the
NumPy reference, compared with `==`."""
import numpy as np
import pytest
import torch

from nm03_capstone_project_amd import ops
from nm03_capstone_project_amd.ops import reference

import intensity_cases as ic

pytestmark = pytest.mark.gpu

CASES_2D = ic.cases_2d()
CASES_3D = ic.cases_3d()


def _dev(mask, raw):
    return torch.from_numpy(mask.astype(bool)).cuda(), torch.from_numpy(raw.view(np.int16)).cuda()


def test_every_2d_case_in_one_launch(native):
    """Every case in ONE batched launch of mixed sizes and sample formats, a workgroup per mask."""
    dev = [_dev(c[1], c[2]) for c in CASES_2D]
    args = ([d[0] for d in dev], [d[1] for d in dev], [c[3] for c in CASES_2D], [c[4] for c in CASES_2D])
    got = ops.measure_intensity(*args)
    assert len(got) == len(CASES_2D)
    for (name, mask, raw, ptype, bits), rec in zip(CASES_2D, got):
        assert rec == native.golden_measure_intensity(mask, raw, ptype, bits), name
        assert rec == reference.measure_intensity(mask, raw, ptype, bits), name
    # the same launch again: nothing is left behind in the records
    assert ops.measure_intensity(*args) == got


def test_2d_tensor_batch_and_single_slice(native):
    r = np.random.default_rng(70)
    mask = r.random((3, 33, 129)) < 0.5
    raw = r.integers(0, 65536, size=mask.shape).astype(np.uint16)
    m, x = _dev(mask, raw)
    got = ops.measure_intensity(m, x)
    assert got == [reference.measure_intensity(mask[i], raw[i]) for i in range(3)]
    assert ops.measure_intensity(m[1], x[1]) == [got[1]]


def test_stray_plane_bits_past_the_width_do_not_count(native):
    """The bit planes as a kernel may find them: every storage bit past the width set."""
    _, mask, raw, ptype, bits = next(c for c in CASES_2D if c[0] == "70x5")
    m, x = _dev(mask, raw)
    h, w = mask.shape
    planes = ops.pack_bits(m.unsqueeze(0)).reshape(h, -1).clone()
    planes[:, -1] |= -1 << (w & 63)
    got = native.k_measure_intensity(planes.data_ptr(), x.data_ptr(), [h], [w], [ptype], [bits],
                                     torch.cuda.current_stream().cuda_stream)
    assert got == [reference.measure_intensity(mask, raw, ptype, bits)]


@pytest.mark.parametrize("name,mask,raw,ptype,bits", CASES_3D, ids=ic.ids(CASES_3D))
def test_measure_volume_intensity_equals_golden_and_numpy(native, name, mask, raw, ptype, bits):
    m, x = _dev(mask, raw)
    got = ops.measure_volume_intensity(m, x, ptype, bits)
    assert got == native.golden_measure_volume_intensity(mask, raw, ptype, bits)
    assert got == reference.measure_volume_intensity(mask, raw, ptype, bits)
    assert got == ops.measure_volume_intensity(m, x, ptype, bits)  # the accumulators are reset by the first launch


def test_2d_and_3d_agree_on_one_plane(native):
    _, mask, raw, ptype, bits = next(c for c in CASES_2D if c[0] == "256x300_second_trip")
    m, x = _dev(mask, raw)
    assert ops.measure_volume_intensity(m.unsqueeze(0), x.unsqueeze(0), ptype, bits) == ops.measure_intensity(m, x, ptype, bits)[0]


def test_ops_reject_bad_arguments():
    m = torch.zeros((3, 4), dtype=torch.bool, device="cuda")
    raw = torch.zeros((3, 4), dtype=torch.int16, device="cuda")
    with pytest.raises(ValueError):
        ops.measure_intensity(m, raw[:2])
    with pytest.raises(ValueError):
        ops.measure_intensity(m, raw.float())
    with pytest.raises(ValueError):
        ops.measure_intensity(m.cpu(), raw)
    with pytest.raises(ValueError):
        ops.measure_intensity(m, raw, stored_bits=17)
    with pytest.raises(ValueError):
        ops.measure_intensity([], [])
    with pytest.raises(ValueError):
        ops.measure_intensity([m, m], [raw, raw], ["u16"], [16, 16])  # one entry per slice
    with pytest.raises(ValueError):
        ops.measure_intensity(m, raw, pixel_type="f32")
    with pytest.raises(ValueError):
        ops.measure_volume_intensity(m, raw)
    with pytest.raises(ValueError):
        ops.measure_volume_intensity(m.unsqueeze(0), raw.unsqueeze(0)[:, :2])
    assert ops.measure_volume_intensity(m.unsqueeze(0), raw.unsqueeze(0))["count"] == 0


# ---------------------------------------------------------------------------------------------
# SlicePipeline / run_array
# ---------------------------------------------------------------------------------------------
def _slices(native):
    return [native.phantom_slice(256, 256, p, s, 25, 7) for p, s in ((3, 12), (1, 10))]


def test_run_array_with_and_without_the_flag(native):
    import nm03_capstone_project_amd as nm
    on = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure_intensity=True))
    off = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure=True))
    both = nm.SlicePipeline(nm.PipelineConfig(batch_size=2, streams=1, measure_intensity=True, measure_diameters=True))
    meta = {"type": "u16", "stored_bits": 16, "slope": 2.0, "intercept": -100.0, "spacing_x": 0.5, "spacing_y": 0.75}
    some = 0
    for raw in _slices(native):
        raw = np.ascontiguousarray(raw, dtype=np.uint16)
        r, g = on.run_array(raw, meta), on.golden(raw, meta)
        assert r["intensity"] == g["intensity"] and r["measure_json"] == g["measure_json"] and r["measure"] == g["measure"]
        assert r["intensity"] == reference.measure_intensity(r["dilated"], raw, "u16", 16)
        assert r["intensity"]["count"] == r["measure"]["area_px"]
        some += r["intensity"]["count"] > 0
        r0, g0 = off.run_array(raw, meta), off.golden(raw, meta)
        assert "intensity" not in r0 and "intensity" not in g0 and r0["measure_json"] == g0["measure_json"]
        assert r["measure_json"].startswith(r0["measure_json"][:-2] + ',"raw_sum_sq":')
        rb, gb = both.run_array(raw, meta), both.golden(raw, meta)
        assert rb["measure_json"] == gb["measure_json"] and rb["intensity"] == r["intensity"]
        assert rb["diameters"] == gb["diameters"]
    assert some == 2, "empty masks prove nothing"


# ---------------------------------------------------------------------------------------------
# VolumePipeline(measure=True, measure_intensity=True)
# ---------------------------------------------------------------------------------------------
def test_volume_pipeline_equals_golden_measure(native):
    import nm03_capstone_project_amd as nm
    import volume_cases as vc
    vol = vc.serpentine_volume(**vc.SERPENTINE)
    spacing = (0.5, 0.75, 2.5)
    kw = dict(spacing=spacing, spacing_z_source="spacing_between_slices")
    vp = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_intensity=True)
    res = vp.run(vol, **kw)
    rec, text, intensity = vp.golden_measure(res["dilated"], res["region"], vol, **kw)
    assert res["intensity"] == intensity and res["measure_json"] == text and res["measure"] == rec
    assert intensity == reference.measure_volume_intensity(res["dilated"], vol) and intensity["count"] == rec["volume_vox"] > 0
    off = nm.VolumePipeline(connectivity=6, dilation=7, measure=True)
    res0 = off.run(vol, **kw)
    assert "intensity" not in res0 and res0["measure_json"] == off.golden_measure(res["dilated"], res["region"], vol, **kw)[1]
    assert text.startswith(res0["measure_json"][:-2] + ',"raw_sum_sq":')
    vl = nm.VolumePipeline(connectivity=6, dilation=7, measure=True, measure_lesions=2, measure_intensity=True)
    resl = vl.run(vol, **kw)
    recl, textl, lesions, intl = vl.golden_measure(resl["dilated"], resl["region"], vol, **kw)
    assert (resl["measure"], resl["measure_json"], resl["lesions"], resl["intensity"]) == (recl, textl, lesions, intl)
    assert intl == intensity and textl.startswith(text[:-2] + ',"lesions_max":2,')


def test_run_slab_refuses_intensity(native):
    vol = np.zeros((4, 16, 64), np.uint16)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError, match="slabs"):
        runner.run_slab(native.self_comm(), vol, 0, 4, native.PipelineParams(), 6, 3, [], measure_intensity=True)
    with pytest.raises(ValueError):
        runner.run(vol, native.PipelineParams(), 6, 3, [], measure_intensity=True)  # needs measure


# ---------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------
import os  # noqa: E402

from conftest import run_bin  # noqa: E402


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def two_patients(tmp_path_factory, native):
    root = str(tmp_path_factory.mktemp("gidata")) + "/"
    native.synth_cohort(root, patients=2, min_slices=3, max_slices=3, threads=2)
    return root


def _cli(data, out, *args):
    r = run_bin("img_processing_parallel", "--quiet", *args, "--data-root", data, "--out", str(out))
    assert r.returncode == 0, r.stderr
    return tree(out)


def test_cli_2d_gpu_equals_cpu(two_patients, tmp_path):
    cpu = _cli(two_patients, tmp_path / "cpu", "--cpu", "--measure-intensity")
    gpu = _cli(two_patients, tmp_path / "gpu", "--measure-intensity")
    names = [k for k in gpu if k.endswith("_measure.json")]
    assert len(names) == 6 and "measurements.csv" in gpu
    assert all(gpu[k] == cpu[k] for k in names) and gpu["measurements.csv"] == cpu["measurements.csv"]
    assert set(gpu) == set(cpu)


def test_cli_3d_gpu_equals_cpu(two_patients, tmp_path):
    cpu = _cli(two_patients, tmp_path / "cpu", "--mode", "3d", "--cpu", "--measure-intensity")
    gpu = _cli(two_patients, tmp_path / "gpu", "--mode", "3d", "--measure-intensity")
    names = [k for k in gpu if k.endswith("volume_measure.json")]
    assert len(names) == 2 and all(gpu[k] == cpu[k] for k in names) and gpu["volumes.csv"] == cpu["volumes.csv"]
    assert b'"raw_p50":' in gpu[names[0]] and set(gpu) == set(cpu)
