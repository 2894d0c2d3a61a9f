"""examples/volume_3d.py --mesh DIR writes mesh.ply and mesh.json (needs the GPU, as the example does)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import volume_export_cases as xc
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture
def volume(native):
    d, h, w = 5, 104, 136
    s0 = xc.slice0(d)
    return np.stack([native.phantom_slice(h, w, 3, s0 + k, xc.NSLICES, xc.SEED) for k in range(d)]).astype(np.uint16)


def test_volume_3d_example_mesh(native, volume, tmp_path):
    from nm03_capstone_project_amd.utils import read_volume_mesh
    sdir = tmp_path / "series"
    os.makedirs(sdir)
    for z, plane in enumerate(volume):
        with open(sdir / f"1-{z + 1}.dcm", "wb") as f:
            f.write(native.dicom_bytes(plane, instance=z + 1, type="u16", bits_stored=16, write_rescale=False, slope=1.0,
                                       intercept=0.0, spacing_x=0.5, spacing_y=0.5))
    out = tmp_path / "mesh"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "volume_3d.py"), "--series", str(sdir), "--mesh", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == ["mesh.json", "mesh.ply"]
    rec = json.load(open(out / "mesh.json"))
    m = read_volume_mesh(str(out))
    assert rec["vertices"] == len(m["vertices"]) > 0 and rec["triangles"] == len(m["triangles"])
    assert rec["bytes"] == os.path.getsize(out / "mesh.ply") and rec["spacing"][:2] == [0.5, 0.5]
    assert f"mesh: {rec['vertices']} vertices, {len(m['quads'])} quads" in r.stdout
