"""examples/volume_3d.py --dilate-mm R prints the voxel counts of the margin and of the default cube, and the thickness
(needs the GPU, as the example does)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import volume_export_cases as xc
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_volume_3d_example_dilate_mm(native, tmp_path):
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
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "volume_3d.py"), "--series", str(sdir), "--dilate-mm", "2.5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "GPU == golden: True" in r.stdout
    g = nm.utils.series_geometry(str(sdir))
    um = list(native.volume_spacing_um(float(np.float32(g["spacing_x"])), float(np.float32(g["spacing_y"])), g["spacing_z"]))
    pipe = nm.VolumePipeline(nm.PipelineConfig())
    band = pipe.run(volume)["band"]
    region, cube = pipe.golden(band, pipe.default_seeds(band))
    margin = native.golden_dilate3d_mm(region, um, 2500)
    m = re.search(r"margin of 2\.5 mm at .*: (\d+) voxels; the 7x7x7 cube: (\d+) voxels", r.stdout)
    assert m and (int(m.group(1)), int(m.group(2))) == (int(margin.sum()), int(cube.sum())) and int(margin.sum()) > 0
    t = native.golden_volume_thickness(margin, um)
    assert f"thickness {t['thickness_mm']:.3f} mm (inscribed radius {t['inscribed_radius_mm']:.3f} mm at " \
           f"{tuple(t['inscribed_at'])})" in r.stdout
