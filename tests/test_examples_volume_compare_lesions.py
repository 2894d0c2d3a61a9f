"""examples/volume_3d.py --dilate-mm R --compare-to-cube --compare-lesions N also prints the lesion-wise totals of the
margin's mask against the default cube's (needs the GPU, as the example does)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import volume_export_cases as xc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_volume_3d_example_compare_lesions(native, tmp_path):
    import nm03_capstone_project_amd as nm
    d, h, w = 5, 104, 136
    s0 = xc.slice0(d)
    volume = np.stack([native.phantom_slice(h, w, 3, s0 + k, xc.NSLICES, xc.SEED) for k in range(d)]).astype(np.uint16)
    sdir = tmp_path / "series"
    os.makedirs(sdir)
    for z, plane in enumerate(volume):
        with open(sdir / f"1-{z + 1}.dcm", "wb") as f:
            f.write(native.dicom_bytes(plane, instance=z + 1, type="u16", bits_stored=16, write_rescale=False, slope=1.0,
                                       intercept=0.0, spacing_x=0.5, spacing_y=0.5))
    script = os.path.join(ROOT, "examples", "volume_3d.py")
    r = subprocess.run([sys.executable, script, "--series", str(sdir), "--dilate-mm", "2.5", "--compare-to-cube", "--compare-lesions", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GPU == golden: True" in r.stdout and "margin against the cube: Dice" in r.stdout
    g = nm.utils.series_geometry(str(sdir))
    um = list(native.volume_spacing_um(float(np.float32(g["spacing_x"])), float(np.float32(g["spacing_y"])), g["spacing_z"]))
    pipe = nm.VolumePipeline(nm.PipelineConfig())
    band = pipe.run(volume)["band"]
    region, cube = pipe.golden(band, pipe.default_seeds(band))
    margin = native.golden_dilate3d_mm(region, um, 2500)
    rec = native.golden_compare_volume_lesions(margin, cube, 4, 26)
    c = json.loads(native.volume_compare_to_json(native.golden_compare_volumes(margin, cube, um), w, h, d, um, "cube", rec))
    assert rec["lesions_a"] >= 1 and rec["hit_b"] >= 1
    assert (f"lesions (connectivity 26): margin {rec['lesions_a']} ({rec['hit_a']} hit, {rec['multi_a']} merging), "
            f"cube {rec['lesions_b']} ({rec['hit_b']} hit, {rec['multi_b']} split), F1 {c['lesion_f1']:.4f}") in r.stdout


def test_example_flag_needs_compare_to_cube(tmp_path):
    script = os.path.join(ROOT, "examples", "volume_3d.py")
    r = subprocess.run([sys.executable, script, "--series", str(tmp_path), "--dilate-mm", "2.5", "--compare-lesions", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--compare-lesions needs --compare-to-cube" in r.stderr
