"""examples/volume_3d.py --views DIR writes the twelve view files and the sidecar (needs the GPU, as the example does)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import volume_export_cases as xc
from conftest import ROOT

pytestmark = pytest.mark.gpu

VIEW_NAMES = ("view_axial", "view_coronal", "view_sagittal", "mip_axial", "mip_coronal", "mip_sagittal")
FILES = tuple(f"{v}_{k}.jpg" for v in VIEW_NAMES for k in ("original", "processed"))


@pytest.fixture
def volume(native):
    d, h, w = 5, 104, 136
    s0 = xc.slice0(d)
    return np.stack([native.phantom_slice(h, w, 3, s0 + k, xc.NSLICES, xc.SEED) for k in range(d)]).astype(np.uint16)


def test_volume_3d_example_views(native, volume, tmp_path):
    sdir = tmp_path / "series"
    os.makedirs(sdir)
    for z, plane in enumerate(volume):
        with open(sdir / f"1-{z + 1}.dcm", "wb") as f:
            f.write(native.dicom_bytes(plane, instance=z + 1, type="u16", bits_stored=16, write_rescale=False, slope=1.0,
                                       intercept=0.0, spacing_x=0.5, spacing_y=0.5))
    out = tmp_path / "views"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "volume_3d.py"), "--series", str(sdir), "--views", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(out)) == sorted(FILES + ("views.json",))
    rec = json.load(open(out / "views.json"))
    assert (rec["width"], rec["height"], rec["depth"]) == (136, 104, 5) and f"views through {tuple(rec['at'])}" in r.stdout
