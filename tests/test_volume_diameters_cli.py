"""--measure-volume-diameters above the kernels, on the CPU: the sidecar text (byte-identical to the unflagged
text once the new keys are removed), VolumePipeline.golden_measure, lesions.csv and its reader, the --cpu CLI
at one and two ranks, --resume, and the refusals."""
import json
import os

import numpy as np
import pytest

import volume_diameter_cases as vdc
import volume_lesion_cases as vlc
from conftest import run_bin

DOUBLE_KEYS = ("diameter_3d_mm", "axial_major_mm", "axial_perp_mm", "axial_bidimensional_mm2")
NEW_COLUMNS = ("major_um2,major_xa,major_ya,major_za,major_xb,major_yb,major_zb,axial_z,axial_um2,axial_xa,axial_ya,axial_xb,"
               "axial_yb,axial_perp_extent,axial_perp_xc,axial_perp_yc,axial_perp_xd,axial_perp_yd,diameter_3d_mm,axial_major_mm,"
               "axial_perp_mm,axial_bidimensional_mm2")
strip_new_keys, tree = vdc.strip_new_keys, vdc.tree


def _fmt9(v):
    return float("%.9g" % v)


def check_derived(obj, um):
    ra = np.sqrt(float(obj["axial_um2"]))
    assert obj["diameter_3d_mm"] == _fmt9(np.sqrt(float(obj["major_um2"])) / 1000.0)
    assert obj["axial_major_mm"] == _fmt9(ra / 1000.0)
    perp = um[0] * um[1] * obj["axial_perp_extent"] / ra / 1000.0 if obj["axial_um2"] else 0.0
    assert obj["axial_perp_mm"] == _fmt9(perp)
    assert obj["axial_bidimensional_mm2"] == _fmt9(ra / 1000.0 * perp)


def test_sidecar_text_with_diameters(native):
    mask = vlc.word_straddle(130)
    mask[0, 0, 0] = 1
    region, raw = vlc.inputs(mask)
    rec = native.golden_measure_volume(mask, region, raw, "u16", 16, 26)
    les = native.golden_measure_volume_lesions(mask, raw, 5, "u16", 16, 26)
    args = (130, 9, 6, 0.977, 1.02, 3.3, "position", 2.0, -5.0, True, 26)
    um = native.volume_spacing_um(float(np.float32(0.977)), float(np.float32(1.02)), 3.3)
    assert um == (977, 1020, 3300)
    dia = native.golden_measure_volume_diameters(mask, 5, um, 26)
    plain = native.volume_measure_to_json(rec, *args, les, 5)
    text = native.volume_measure_to_json(rec, *args, les, 5, diameters=dia)
    assert text != plain and strip_new_keys(text) == plain and text.count("\n") == 1
    assert native.volume_measure_to_json(rec, *args, les, 5, diameters=dia, spacing_um=um) == text
    d, p = json.loads(text), json.loads(plain)
    keys = list(d)
    assert keys[keys.index("diameters_spacing_um") + 1] == "lesions_max" and d["diameters_spacing_um"] == list(um)
    assert [k for k in keys if k != "diameters_spacing_um"] == list(p)
    assert len(d["lesions"]) == 3 == len(dia)
    for obj, old, rec_d in zip(d["lesions"], p["lesions"], dia):
        assert list(obj) == list(old) + list(vdc.INT_KEYS) + list(DOUBLE_KEYS)
        assert {k: obj[k] for k in vdc.INT_KEYS} == rec_d
        check_derived(obj, um)
    # with the intensity and texture keys the new ones still stand where they belong
    inten = native.golden_measure_volume_intensity(mask, raw, "u16", 16)
    full_plain = native.volume_measure_to_json(rec, *args, les, 5, inten)
    full = native.volume_measure_to_json(rec, *args, les, 5, inten, diameters=dia)
    assert strip_new_keys(full) == full_plain and ',"diameters_spacing_um":[977,1020,3300],"lesions_max":5' in full
    # the one-voxel lesion: zeros, and 0 for the perpendicular
    speck = d["lesions"][-1]
    assert speck["voxels"] == 1 and all(speck[k] == 0 for k in DOUBLE_KEYS)
    with pytest.raises(ValueError):
        native.volume_measure_to_json(rec, *args, les, 5, diameters=dia[:2])
    with pytest.raises(ValueError):
        native.volume_measure_to_json(rec, *args, diameters=dia)  # no lesions
    e = native.volume_measure_to_json(rec, *args, [], 3, diameters=[])
    assert e.endswith(',"diameters_spacing_um":[977,1020,3300],"lesions_max":3,"lesions":[]}\n')


def test_hand_values_in_the_sidecar(native):
    m = vdc.hand_box()
    raw = np.zeros(m.shape, np.uint16)
    rec = native.golden_measure_volume(m, m, raw, "u16", 16, 26)
    les = native.golden_measure_volume_lesions(m, raw, 1, "u16", 16, 26)
    dia = native.golden_measure_volume_diameters(m, 1)
    obj = json.loads(native.volume_measure_to_json(rec, 12, 6, 4, 1.0, 1.0, 1.0, "default", 1.0, 0.0, True, 26, les, 1,
                                                   diameters=dia))["lesions"][0]
    assert {k: obj[k] for k in vdc.INT_KEYS} == vdc.HAND
    assert obj["diameter_3d_mm"] == _fmt9(np.sqrt(94.0)) and obj["axial_major_mm"] == _fmt9(np.sqrt(90.0))
    assert obj["axial_perp_mm"] == pytest.approx(5.6921, abs=1e-4)
    assert obj["axial_bidimensional_mm2"] == 54.0


def test_pipeline_golden_measure_with_diameters(native):
    import nm03_capstone_project_amd as nm
    mask = vlc.equal_boxes()
    region, raw = vlc.inputs(mask)
    sp = (0.5, 0.5, 5.0)
    vp = nm.VolumePipeline(measure=True, measure_lesions=4, measure_diameters=True)
    rec, text, lesions, dia = vp.golden_measure(mask, region, raw, spacing=sp)
    assert dia == native.golden_measure_volume_diameters(mask, 4, (500, 500, 5000), 26) and len(dia) == 2
    plain = nm.VolumePipeline(measure=True, measure_lesions=4).golden_measure(mask, region, raw, spacing=sp)
    assert plain == (rec, strip_new_keys(text), lesions) and text != plain[1]
    both = nm.VolumePipeline(measure=True, measure_lesions=4, measure_intensity=True, measure_texture=True, measure_diameters=True)
    out = both.golden_measure(mask, region, raw, spacing=sp)
    assert len(out) == 6 and out[-1] == dia and json.loads(out[1])["diameters_spacing_um"] == [500, 500, 5000]
    for bad in (dict(measure_diameters=True), dict(measure=True, measure_diameters=True)):
        with pytest.raises(ValueError):
            nm.VolumePipeline(**bad)


# ---------------------------------------------------------------------------------------------
# CLI on the golden model
# ---------------------------------------------------------------------------------------------
def _cli(cohort_root, out, *args):
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--quiet", *args, "--data-root", cohort_root, "--out",
                str(out), "--json", str(out) + ".json")
    assert r.returncode == 0, r.stderr
    return tree(out)


@pytest.fixture(scope="module")
def cpu_trees(cohort_root, tmp_path_factory):
    base = tmp_path_factory.mktemp("vdcpu")
    return (base / "dia", _cli(cohort_root, base / "dia", "--measure-volume-lesions", "3", "--measure-volume-diameters"),
            _cli(cohort_root, base / "les", "--measure-volume-lesions", "3"), base / "les")


def test_cli_cpu_sidecars_and_table(native, cohort_root, cpu_trees):
    from nm03_capstone_project_amd.utils import read_volume_lesions
    out, dia, les, les_out = cpu_trees
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    # Everything but the sidecars and lesions.csv is what the run without the flag writes.
    assert set(dia) == set(les)
    differing = sorted(k for k in les if dia[k] != les[k])
    assert differing == sorted(["lesions.csv"] + [os.path.join(p, "volume_measure.json") for p in pids])
    assert dia["volumes.csv"] == les["volumes.csv"]
    old_header = les["lesions.csv"].decode().splitlines()[0]
    assert dia["lesions.csv"].decode().splitlines()[0] == old_header + "," + NEW_COLUMNS
    # lesions.csv without the new columns is the unflagged table
    ncols = old_header.count(",") + 1
    assert "\n".join(",".join(line.split(",")[:ncols]) for line in dia["lesions.csv"].decode().splitlines()) + "\n" == \
        les["lesions.csv"].decode()
    rows = read_volume_lesions(str(out))
    old_rows = read_volume_lesions(str(les_out))
    assert len(rows) == len(old_rows) > 0
    at, d3max = 0, 0.0
    for pid in pids:
        text = dia[os.path.join(pid, "volume_measure.json")].decode()
        assert strip_new_keys(text) == les[os.path.join(pid, "volume_measure.json")].decode()
        d = json.loads(text)
        um = d["diameters_spacing_um"]
        assert um == list(native.volume_spacing_um(d["spacing_x"], d["spacing_y"], d["spacing_z"]))
        for obj in d["lesions"]:
            r, old = rows[at], old_rows[at]
            at += 1
            assert vdc.pair_holds(obj, um)
            check_derived(obj, um)
            x0, y0, z0, x1, y1, z1 = obj["bbox"]
            assert all(x0 <= obj["major"][k] <= x1 and y0 <= obj["major"][k + 1] <= y1 and z0 <= obj["major"][k + 2] <= z1
                       for k in (0, 3))
            assert {k: r[k] for k in old} == old and r["patient"] == pid
            assert [r[f"major_{c}"] for c in ("xa", "ya", "za", "xb", "yb", "zb")] == obj["major"]
            assert [r[f"axial_{c}"] for c in ("xa", "ya", "xb", "yb")] == obj["axial"]
            assert [r[f"axial_perp_{c}"] for c in ("xc", "yc", "xd", "yd")] == obj["axial_perp"]
            assert all(r[k] == obj[k] for k in ("major_um2", "axial_z", "axial_um2", "axial_perp_extent") + DOUBLE_KEYS)
            d3max = max(d3max, obj["diameter_3d_mm"])
    assert at == len(rows)
    js = json.load(open(str(out) + ".json"))["measure_volume"]
    assert js["diameters"] is True and js["diameter_3d_mm_max"] == d3max > 0
    old_js = json.load(open(str(les_out) + ".json"))["measure_volume"]
    assert "diameters" not in old_js and {k: js[k] for k in old_js} == old_js


def test_cli_cpu_two_ranks_same_tree(cohort_root, cpu_trees, tmp_path):
    assert _cli(cohort_root, tmp_path / "two", "--measure-volume-lesions", "3", "--measure-volume-diameters", "--gpus",
                "2") == cpu_trees[1]


def test_cli_flag_alone_implies_one_lesion(cohort_root, cpu_trees, tmp_path):
    one = _cli(cohort_root, tmp_path / "one", "--measure-volume-diameters")
    plain = _cli(cohort_root, tmp_path / "plain", "--measure-volume-lesions", "1")
    assert set(one) == set(plain) and strip_new_keys(one[sorted(k for k in one if k.endswith("volume_measure.json"))[0]].decode()) \
        == plain[sorted(k for k in plain if k.endswith("volume_measure.json"))[0]].decode()
    d = json.loads(one[sorted(k for k in one if k.endswith("volume_measure.json"))[0]])
    assert d["lesions_max"] == 1 and "major_um2" in d["lesions"][0]
    # the first lesion's record does not depend on N
    first = json.loads(cpu_trees[1][sorted(k for k in one if k.endswith("volume_measure.json"))[0]])["lesions"][0]
    assert d["lesions"][0] == first


def test_cli_resume_writes_the_same_tree(cohort_root, cpu_trees, tmp_path):
    """3D mode recomputes every patient under --resume as without it; a sidecar written earlier without the flag
    is overwritten with the flagged one."""
    out = tmp_path / "again"
    assert _cli(cohort_root, out, "--measure-volume-lesions", "3") == cpu_trees[2]
    assert _cli(cohort_root, out, "--measure-volume-lesions", "3", "--measure-volume-diameters", "--resume") == cpu_trees[1]


@pytest.mark.parametrize("args,word", [
    (("--measure-volume-diameters",), "--measure-volume-diameters needs --mode 3d"),
    (("--mode", "3d", "--measure-volume-diameters", "--split-volume"),
     "--measure-volume-diameters is not available with --split-volume"),
    (("--mode", "3d", "--measure-diameters"), "--measure-diameters is not available with --mode 3d"),
])
def test_cli_rejections(cohort_root, tmp_path, args, word):
    out = tmp_path / "o"
    r = run_bin("img_processing_parallel", "--cpu", "--data-root", cohort_root, "--out", str(out), *args)
    assert r.returncode == 2 and word in r.stderr
    assert not out.exists()


def test_flag_in_help_and_bench():
    r = run_bin("img_processing_parallel", "--help")
    assert r.returncode == 0 and "--measure-volume-diameters" in r.stdout
    r = run_bin("nm03_bench", "--config", "volume", "--measure-volume-diameters")
    assert r.returncode == 2 and "--measure-volume-diameters needs --measure-volume-lesions" in r.stderr
