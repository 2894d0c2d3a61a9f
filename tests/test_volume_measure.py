"""--measure-volume without a GPU: the golden model against the SciPy reference and against the host
run of the K8 kernels' word arithmetic, the slice spacing, the sidecar text and the --cpu CLI."""
import json
import os

import numpy as np
import pytest

import volume_measure_cases as vmc
from conftest import run_bin

CASES = vmc.all_cases()
CONNS = (6, 26)


def _tunnels(rec):
    return rec["components"] + rec["cavities"] - rec["euler"]


# ---------------------------------------------------------------------------------------------
# golden == reference == the kernels' word arithmetic on the host
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_golden_equals_reference_and_word_arithmetic(native, name, build, conn):
    from nm03_capstone_project_amd.ops import reference
    mask = build()
    region, raw = vmc.region_for(mask), vmc.raw_for(mask.shape)
    gold = native.golden_measure_volume(mask, region, raw, "u16", 16, conn)
    ref = reference.measure_volume(mask, region, raw, conn, "u16", 16)
    assert gold == ref
    assert native.measure_volume_words(mask, region, raw, "u16", 16, conn) == gold
    assert _tunnels(gold) >= 0
    assert gold["region_vox"] == int(region.sum()) and gold["volume_vox"] == int(mask.sum())


@pytest.mark.parametrize("name", list(vmc.SOLIDS))
def test_topology_of_the_named_solids(native, name):
    build, expected = vmc.SOLIDS[name]
    mask = build()
    raw = vmc.raw_for(mask.shape)
    for conn, (comps, cavities, tunnels) in expected.items():
        rec = native.golden_measure_volume(mask, mask, raw, "u16", 16, conn)
        assert (rec["components"], rec["cavities"], _tunnels(rec)) == (comps, cavities, tunnels), conn


def test_trivial_volumes(native):
    shape = (3, 4, 66)
    raw = vmc.raw_for(shape)
    for conn in CONNS:
        e = native.golden_measure_volume(vmc.empty(shape), vmc.empty(shape), raw, "u16", 16, conn)
        assert e["volume_vox"] == 0 and e["bbox"] == [-1] * 6 and e["components"] == e["cavities"] == e["euler"] == 0
        assert (e["raw_sum"], e["raw_min"], e["raw_max"]) == (0, 0, 0)
        f = native.golden_measure_volume(vmc.full(shape), vmc.full(shape), raw, "u16", 16, conn)
        assert f["volume_vox"] == 3 * 4 * 66 and f["bbox"] == [0, 0, 0, 65, 3, 2]
        assert (f["components"], f["cavities"], f["euler"]) == (1, 0, 1)
        assert (f["faces_x"], f["faces_y"], f["faces_z"]) == (2 * 3 * 4, 2 * 3 * 66, 2 * 4 * 66)
        c = native.golden_measure_volume(vmc.corners(shape), vmc.empty(shape), raw, "u16", 16, conn)
        assert (c["components"], c["largest_vox"], c["cavities"], c["euler"], c["region_vox"]) == (8, 1, 0, 8, 0)


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("which", ["maze", "staircase"])
def test_one_voxel_paths_word_arithmetic(native, which, conn):
    """The deepest union chains: one component however the unions are ordered."""
    mask = getattr(vmc, which)()
    raw = vmc.raw_for(mask.shape)
    gold = native.golden_measure_volume(mask, mask, raw, "u16", 16, conn)
    assert gold["components"] == 1 and gold["largest_vox"] == int(mask.sum())
    assert native.measure_volume_words(mask, mask, raw, "u16", 16, conn) == gold


# ---------------------------------------------------------------------------------------------
# intensity statistics
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ptype,bits", [("i16", 16), ("u16", 12), ("i16", 12)])
def test_intensity_statistics_against_numpy(native, ptype, bits):
    shape = (5, 9, 70)
    mask = vmc.noise(shape, 0.31)
    raw = vmc.raw_for(shape, seed=bits)
    v = raw.astype(np.int64)
    if ptype == "i16":
        sh = 16 - bits
        v = ((v << sh) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.int64) >> sh
        assert v.min() < 0 < v.max()
    else:
        v = v & ((1 << bits) - 1)
    under = v[mask.astype(bool)]
    for fn in (native.golden_measure_volume, native.measure_volume_words):
        rec = fn(mask, mask, raw, ptype, bits, 26)
        assert (rec["raw_sum"], rec["raw_min"], rec["raw_max"]) == (int(under.sum()), int(under.min()), int(under.max()))


# ---------------------------------------------------------------------------------------------
# slice spacing
# ---------------------------------------------------------------------------------------------
def _write_series(native, root, specs):
    os.makedirs(root, exist_ok=True)
    px = np.arange(16 * 24, dtype=np.uint16).reshape(16, 24)
    for i, kw in enumerate(specs):
        with open(os.path.join(root, f"1-{i + 1}.dcm"), "wb") as f:
            f.write(native.dicom_bytes(px + i, instance=i + 1, spacing_x=0.5, spacing_y=0.75, **kw))
    return str(root)


def test_series_geometry_sources(native, tmp_path):
    from nm03_capstone_project_amd.utils import series_geometry
    # 1. ImagePositionPatient of the first two slices, an oblique step of length 5; the other tags lose.
    d = _write_series(native, tmp_path / "pos", [dict(position=[1.0, 2.0, 3.0], slice_thickness=2.0, spacing_between_slices=2.5),
                                                 dict(position=[1.0, 5.0, 7.0], slice_thickness=2.0, spacing_between_slices=2.5),
                                                 dict(position=[1.0, 8.0, 11.0])])
    g = series_geometry(d)
    assert (g["spacing_z"], g["spacing_z_source"]) == (5.0, "position")
    assert (g["spacing_x"], g["spacing_y"]) == (0.5, 0.75)
    # 2. Equal positions (distance 0): SpacingBetweenSlices before SliceThickness.
    d = _write_series(native, tmp_path / "sbs", [dict(slice_thickness=3.0, spacing_between_slices=2.5)] * 2)
    g = series_geometry(d)
    assert (g["spacing_z"], g["spacing_z_source"]) == (2.5, "spacing_between_slices")
    # 3. No positions, no SpacingBetweenSlices: SliceThickness.
    d = _write_series(native, tmp_path / "thick", [dict(slice_thickness=3.0, write_position=False)] * 2)
    g = series_geometry(d)
    assert (g["spacing_z"], g["spacing_z_source"]) == (3.0, "slice_thickness")
    # 4. Nothing: 1.0.
    d = _write_series(native, tmp_path / "none", [dict(slice_thickness=0.0, write_position=False)] * 2)
    g = series_geometry(d)
    assert (g["spacing_z"], g["spacing_z_source"]) == (1.0, "default")
    # A single slice has no second position to measure against.
    d = _write_series(native, tmp_path / "one", [dict(position=[0.0, 0.0, 9.0], slice_thickness=4.0)])
    g = series_geometry(d)
    assert (g["spacing_z"], g["spacing_z_source"]) == (4.0, "slice_thickness")


def test_series_geometry_of_the_synthetic_cohort(native, cohort_root):
    from nm03_capstone_project_amd.utils import series_geometry
    base = native.cohort_dir(cohort_root)
    for pid in native.find_patient_dirs(base):
        series_dir, files = native.list_patient_series(base, pid)
        g = series_geometry(series_dir)
        assert (g["spacing_z"], g["spacing_z_source"]) == (5.0, "position")
        assert g["spacing_x"] == g["spacing_y"] == 0.9375
        assert native.series_geometry(files) == g


def test_read_slice_keys_unchanged(native, cohort_root):
    base = native.cohort_dir(cohort_root)
    _, files = native.list_patient_series(base, native.find_patient_dirs(base)[0])
    _, meta = native.read_slice(files[0], 0, -1)
    assert not any("thickness" in k or "spacing_z" in k or "between" in k for k in meta)


# ---------------------------------------------------------------------------------------------
# the sidecar text
# ---------------------------------------------------------------------------------------------
KEYS = ["width", "height", "depth", "connectivity", "volume_vox", "region_vox", "bbox", "sum_x", "sum_y", "sum_z",
        "faces_x", "faces_y", "faces_z", "components", "largest_vox", "cavities", "euler", "raw_sum", "raw_min", "raw_max",
        "tunnels", "spacing_x", "spacing_y", "spacing_z", "spacing_z_source", "volume_mm3", "volume_ml", "surface_mm2",
        "centroid_x", "centroid_y", "centroid_z", "centroid_x_mm", "centroid_y_mm", "centroid_z_mm", "mean"]


def test_volume_to_json_keys_nulls_and_mm3(native):
    mask = vmc.torus()
    raw = np.full(mask.shape, 100, np.uint16)
    rec = native.golden_measure_volume(mask, mask, raw, "u16", 16, 26)
    text = native.volume_measure_to_json(rec, 41, 41, 21, 0.5, 0.25, 3.0, "position", 2.0, -5.0, True, 26)
    assert text.endswith("}\n") and text.count("\n") == 1
    d = json.loads(text)
    assert list(d) == KEYS
    n = rec["volume_vox"]
    assert d["volume_mm3"] == pytest.approx(n * 0.5 * 0.25 * 3.0, rel=1e-8) and d["volume_ml"] == pytest.approx(d["volume_mm3"] / 1000)
    assert d["surface_mm2"] == pytest.approx(rec["faces_x"] * 0.25 * 3.0 + rec["faces_y"] * 0.5 * 3.0 + rec["faces_z"] * 0.5 * 0.25,
                                            rel=1e-8)
    assert d["tunnels"] == 1 and d["bbox"] == rec["bbox"] and d["spacing_z_source"] == "position"
    assert d["centroid_x"] == pytest.approx(20.0) and d["centroid_z_mm"] == pytest.approx(30.0)
    assert d["mean"] == pytest.approx(195.0)  # 100 · 2 − 5
    assert json.loads(native.volume_measure_to_json(rec, 41, 41, 21, 0.5, 0.25, 3.0, "position", 2.0, -5.0, False, 26))["mean"] == 100
    shape = (2, 3, 4)
    e = native.golden_measure_volume(vmc.empty(shape), vmc.empty(shape), vmc.raw_for(shape), "u16", 16, 6)
    d = json.loads(native.volume_measure_to_json(e, 4, 3, 2, 1.0, 1.0, 1.0, "default", 1.0, 0.0, True, 6))
    assert list(d) == KEYS and d["volume_mm3"] == 0 and d["bbox"] == [-1] * 6
    assert all(d[k] is None for k in KEYS[-7:])


# ---------------------------------------------------------------------------------------------
# CLI on the golden model
# ---------------------------------------------------------------------------------------------
def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def cpu_run(cohort_root, tmp_path_factory):
    out = tmp_path_factory.mktemp("vmcpu") / "out"
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--measure-volume", "--quiet", "--data-root", cohort_root,
                "--out", str(out), "--json", str(out) + ".json")
    assert r.returncode == 0, r.stderr
    return out


def test_cli_cpu_sidecars_and_table(native, cohort_root, cpu_run):
    import nm03_capstone_project_amd as nm
    from nm03_capstone_project_amd.utils import read_series, read_volume_measurements, series_geometry
    base = native.cohort_dir(cohort_root)
    pids = native.find_patient_dirs(base)
    vp = nm.VolumePipeline(measure=True)
    rows = read_volume_measurements(str(cpu_run))
    assert [r["patient"] for r in rows] == pids and all(r["status"] == "ok" for r in rows)
    for pid, row in zip(pids, rows):
        series_dir, _ = native.list_patient_series(base, pid)
        vol, slices = read_series(series_dir)
        meta = slices[0].meta
        g = series_geometry(series_dir)
        # The golden 3D pipeline: per-plane band, region growing from the default seeds, 7³ dilation.
        band = np.stack([native.golden_run(vol[z], meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"],
                                           native.PipelineParams())["band"] for z in range(vol.shape[0])])
        region, dil = vp.golden(band, vp.default_seeds(band))
        rec, text = vp.golden_measure(dil, region, vol, spacing=(g["spacing_x"], g["spacing_y"], g["spacing_z"]),
                                      spacing_z_source=g["spacing_z_source"], meta=meta)
        assert (cpu_run / pid / "volume_measure.json").read_text() == text
        d = json.loads(text)
        assert d["spacing_z"] == 5 and d["spacing_z_source"] == "position" and d["spacing_x"] == 0.9375
        assert row["volume_vox"] == rec["volume_vox"] and row["bbox_z1"] == rec["bbox"][5]
        assert row["spacing_z_source"] == "position" and row["volume_mm3"] == d["volume_mm3"]
    assert any(r["volume_vox"] > 0 for r in rows)  # an empty mask proves nothing
    js = json.load(open(str(cpu_run) + ".json"))["measure_volume"]
    assert js["volumes"] == len(pids)
    assert js["volume_vox_total"] == sum(r["volume_vox"] for r in rows)
    assert js["volume_mm3_total"] == pytest.approx(sum(r["volume_mm3"] for r in rows), rel=1e-8)


def test_cli_cpu_leaves_the_jpegs_alone(cohort_root, cpu_run, tmp_path):
    plain = tmp_path / "plain"
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--quiet", "--data-root", cohort_root, "--out", str(plain))
    assert r.returncode == 0, r.stderr
    with_flag, without = tree(cpu_run), tree(plain)
    assert not [k for k in without if k.endswith(".json") or k.endswith(".csv")]
    extra = sorted(set(with_flag) - set(without))
    assert "volumes.csv" in extra and all(k == "volumes.csv" or k.endswith("volume_measure.json") for k in extra)
    assert {k: v for k, v in with_flag.items() if k not in extra} == without


def test_cli_cpu_two_ranks_same_tree(cohort_root, cpu_run, tmp_path):
    out = tmp_path / "two"
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--measure-volume", "--quiet", "--gpus", "2",
                "--data-root", cohort_root, "--out", str(out))
    assert r.returncode == 0, r.stderr
    assert tree(out) == tree(cpu_run)


def test_cli_connectivity_6(native, cohort_root, tmp_path):
    out = tmp_path / "c6"
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--measure-volume", "--measure-volume-connectivity", "6",
                "--quiet", "--data-root", cohort_root, "--out", str(out))
    assert r.returncode == 0, r.stderr
    pid = native.find_patient_dirs(native.cohort_dir(cohort_root))[0]
    assert json.loads((out / pid / "volume_measure.json").read_text())["connectivity"] == 6


@pytest.mark.parametrize("args,word", [(("--measure-volume",), "--measure-volume"),
                                       (("--mode", "3d", "--measure-volume", "--split-volume"), "--measure-volume"),
                                       (("--mode", "3d", "--measure-volume", "--measure-volume-connectivity", "8"),
                                        "--measure-volume-connectivity")])
def test_cli_rejections(cohort_root, tmp_path, args, word):
    out = tmp_path / "o"
    r = run_bin("img_processing_parallel", "--cpu", *args, "--data-root", cohort_root, "--out", str(out))
    assert r.returncode == 2 and word in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("tool", ["img_processing_parallel", "img_processing_sequential", "test_pipeline"])
def test_flags_in_help(tool):
    r = run_bin(tool, "--help")
    assert r.returncode == 0 and "--measure-volume " in r.stdout and "--measure-volume-connectivity 6|26" in r.stdout


def test_pipeline_rejects_other_measure_connectivities():
    import nm03_capstone_project_amd as nm
    assert nm.VolumePipeline().measure is False and nm.VolumePipeline().measure_connectivity == 26
    with pytest.raises(ValueError):
        nm.VolumePipeline(measure=True, measure_connectivity=18)


def test_scratch_words_and_the_32_bit_limit(native):
    assert native.volume_measure_scratch_words(256, 256, 256) == 257 * 256 * 256 + 1
    assert native.volume_measure_scratch_words(65534, 256, 256) == 65535 * 65536 + 1  # the last that fits
    assert native.volume_measure_scratch_words(65535, 256, 256) == 0                  # 2^32 + 1 slots: refused
    assert native.volume_measure_scratch_words(4096, 4096, 4096) == 0
    assert native.volume_measure_scratch_words(0, 5, 5) == 0
