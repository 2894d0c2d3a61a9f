"""Overlap and surface distances between two volume masks (nm03/volume_compare.h, --compare-to, --volume-mask) without
a GPU, everything compared with ==:
  test_models_agree                  golden == SciPy reference == the host run of K17's functions on every case, with
                                     and without junk bits past the width; the surface words against the golden surface
  test_worked_examples               the three worked examples of the header, integer by integer
  test_isqrt                         the shared integer square root around squares up to 2^62
  test_symmetry / test_equal_masks   compare(A, B) <-> compare(B, A); A = B gives dice 1 and all distances 0
  test_sidecar_text_and_csv          the one writer's text, its key order, null rules and the CSV fields
  test_cli_*                         the --cpu tree at one and two ranks, comparisons.csv and its reader, the mask's
                                     round trip, no_reference and shape_mismatch rows, every refusal, and a run
                                     without the flags against the tree it writes today"""
import json
import math
import os
import shutil

import numpy as np
import pytest

import volume_compare_cases as cc
from conftest import run_bin

CASES = cc.cases()


@pytest.fixture(scope="module")
def golden(native):
    """The golden record of every case, computed once."""
    return {c["name"]: native.golden_compare_volumes(c["a"], c["b"], list(c["um"])) for c in CASES}


@pytest.mark.parametrize("c", CASES, ids=cc.ids(CASES))
def test_models_agree(native, golden, c):
    from nm03_capstone_project_amd.ops import reference
    g = golden[c["name"]]
    assert tuple(g) == cc.INTEGER_KEYS
    assert g == reference.compare_volumes(c["a"], c["b"], c["um"])
    assert g == native.volume_compare_words(c["a"], c["b"], list(c["um"]))
    rec, sa, sb = native.volume_compare_words(c["a"], c["b"], list(c["um"]), junk=True, surfaces=True)
    assert g == rec
    d, h, w = c["a"].shape
    for words, mask in ((sa, c["a"]), (sb, c["b"])):
        surf = native.golden_volume_surface(mask)
        assert np.array_equal(surf.astype(bool), reference.volume_surface(mask))
        bits = np.zeros((d, h, words.shape[2] * 64), np.uint8)  # unpack: bits past the width must be zero
        for k in range(words.shape[2]):
            for b in range(64):
                bits[:, :, 64 * k + b] = (words[:, :, k].astype(np.uint64) >> np.uint64(b)) & np.uint64(1)
        assert np.array_equal(bits[:, :, :w], surf) and not bits[:, :, w:].any()
    for k in ("surface_a", "worst_ab", "n_ab", "p95_um_ab", "tp_vox"):  # what the case claims about itself
        if k in c:
            assert g[k] == c[k], k
    if c.get("found") is False:
        assert not g["found_ab"] and not g["found_ba"] and g["worst_ab"] == [-1, -1, -1] == g["worst_ba"]
        assert all(g[k + t] == 0 for k in ("n", "max_um2", "sum_um", "p95_um") for t in ("_ab", "_ba"))
    else:
        assert g["found_ab"] and g["found_ba"] and g["n_ab"] == g["surface_a"] and g["n_ba"] == g["surface_b"]


@pytest.mark.parametrize("name", sorted(cc.WORKED))
def test_worked_examples(native, golden, name):
    g = golden[name]
    for k, v in cc.WORKED[name].items():
        assert g[k] == v, k
    if name == "worked_nested":  # every A→B distance is exactly 3 mm: surface to voxel would give 0
        assert g["sum_um_ab"] == g["n_ab"] * 3000 and g["max_um2_ab"] == 3000 ** 2
    if name == "worked_boxes":
        assert (95 * 104 + 99) // 100 == 99 and (95 * 209 + 99) // 100 == 199


def test_isqrt(native):
    for v, r in cc.WORKED_ISQRT.items():
        assert native.volume_compare_isqrt(v) == r == math.isqrt(v)
    for r in (0, 1, 2, 3, 1000, 94_906_265, 94_906_266, 94_906_267, 2 ** 26, 2 ** 26 + 1, 2 ** 31 - 1, 2_000_000_011, 1_518_500_249):
        for v in (r * r - 1, r * r, r * r + 1, r * r + r, (r + 1) * (r + 1) - 1):
            if 0 <= v < 2 ** 62:
                assert native.volume_compare_isqrt(v) == math.isqrt(v), v
    assert native.volume_compare_isqrt(2 ** 62 - 1) == 2 ** 31 - 1
    with pytest.raises(ValueError):
        native.volume_compare_isqrt(2 ** 62)


@pytest.mark.parametrize("name", ["worked_boxes", "noise_50", "width_65", "a_empty", "single_voxels", "tie_rows"])
def test_symmetry(native, golden, name):
    c = cc.case(name)
    back = native.golden_compare_volumes(c["b"], c["a"], list(c["um"]))
    assert back == cc.swapped(golden[name]) and tuple(back) == cc.INTEGER_KEYS
    assert native.volume_compare_words(c["b"], c["a"], list(c["um"])) == back


def test_equal_masks(native, golden):
    c, g = cc.case("equal"), golden["equal"]
    assert g["tp_vox"] == g["a_vox"] == g["b_vox"] > 0 and g["fp_vox"] == g["fn_vox"] == 0
    for t in ("_ab", "_ba"):
        assert g["max_um2" + t] == g["sum_um" + t] == g["p95_um" + t] == 0 and g["found" + t] and g["n" + t] == g["surface_a"]
    d, h, w = c["a"].shape
    js = json.loads(native.volume_compare_to_json(g, w, h, d, list(c["um"]), "ref"))
    assert js["dice"] == js["jaccard"] == js["sensitivity"] == js["precision"] == 1
    assert js["hausdorff_mm"] == js["hd95_mm"] == js["msd_ab_mm"] == js["msd_ba_mm"] == js["assd_mm"] == 0 == js["volume_diff_mm3"]
    assert g["worst_ab"] == g["worst_ba"]  # the first surface voxel in raster order


def test_sidecar_text_and_csv(native, golden):
    c, g = cc.case("worked_boxes"), golden["worked_boxes"]
    text = native.volume_compare_to_json(g, 16, 8, 5, list(c["um"]), 'dir "x"/PGBM-0001/mask.mhd')
    assert text.endswith("}\n") and text.count("\n") == 1 and " " not in text.replace('dir \\"x\\"', "")
    js = json.loads(text)
    assert tuple(js) == cc.JSON_KEYS
    assert (js["width"], js["height"], js["depth"], js["compare_spacing_um"]) == (16, 8, 5, [1000, 1000, 2500])
    assert js["reference"] == 'dir "x"/PGBM-0001/mask.mhd'
    for k in cc.INTEGER_KEYS:
        assert js[k] == g[k], k  # found_ab / found_ba are written 1 / 0

    def g9(v):
        return float("%.9g" % v)
    assert js["dice"] == g9(2 * 48 / (120 + 289)) and js["jaccard"] == g9(48 / (120 + 289 - 48))
    assert js["sensitivity"] == g9(48 / 289) and js["precision"] == g9(48 / 120)
    vox = 1000 * 1000 * 2500 / 1e9
    assert (js["volume_a_mm3"], js["volume_b_mm3"], js["volume_diff_mm3"]) == (g9(120 * vox), g9(289 * vox), g9((120 - 289) * vox))
    assert js["hausdorff_mm"] == g9(math.sqrt(70_000_000) / 1000) and js["hd95_mm"] == 5.916
    assert js["msd_ab_mm"] == g9(164_741 / 104 / 1000) and js["msd_ba_mm"] == g9(716_543 / 209 / 1000)
    assert js["assd_mm"] == g9((164_741 + 716_543) / (104 + 209) / 1000)
    # the CSV: the same values, arrays flattened, text quoted when it must be
    import csv
    import io
    header = native.volume_compare_csv_header()
    fields = native.volume_compare_csv_fields(g, 16, 8, 5, list(c["um"]), 'dir "x"/PGBM-0001/mask.mhd')
    row = next(csv.DictReader(io.StringIO(header + "\nP,ok," + fields + "\n")))
    assert list(row)[:2] == ["patient", "status"] and row["reference"] == js["reference"]
    flat = []
    for k in cc.JSON_KEYS:
        flat += [k + "_x", k + "_y", k + "_z"] if isinstance(js[k], list) else [k]
    assert list(row)[2:] == flat
    for k in cc.JSON_KEYS:
        if isinstance(js[k], list):
            assert [int(row[k + a]) for a in ("_x", "_y", "_z")] == js[k]
        elif k != "reference":
            assert float(row[k]) == js[k], k
    # null rules: a direction that was not found, and zero denominators
    e = golden["both_empty"]
    js = json.loads(native.volume_compare_to_json(e, 70, 6, 4, [1000, 1000, 1000], ""))
    assert all(js[k] is None for k in ("dice", "jaccard", "sensitivity", "precision", "hausdorff_mm", "hd95_mm", "msd_ab_mm",
                                       "msd_ba_mm", "assd_mm"))
    assert js["volume_a_mm3"] == js["volume_b_mm3"] == js["volume_diff_mm3"] == 0 and js["worst_ab"] == [-1, -1, -1]
    row = next(csv.DictReader(io.StringIO(header + "\nP,ok," + native.volume_compare_csv_fields(e, 70, 6, 4, [1000] * 3, "") + "\n")))
    assert row["dice"] == "" and row["assd_mm"] == "" and row["volume_a_mm3"] == "0" and None not in row and None not in row.values()
    js = json.loads(native.volume_compare_to_json(golden["a_empty"], 70, 6, 4, [1000, 1000, 1000], ""))
    assert js["dice"] == 0 and js["sensitivity"] == 0 and js["precision"] is None and js["hausdorff_mm"] is None


def test_bindings_refuse_bad_arguments(native):
    a = np.zeros((2, 3, 4), np.uint8)
    for fn in (native.golden_compare_volumes, native.volume_compare_words):
        with pytest.raises(ValueError):
            fn(a, np.zeros((2, 3, 5), np.uint8))
        with pytest.raises(ValueError):
            fn(a[0], a[0])
        with pytest.raises(ValueError):
            fn(a, a, [0, 1000, 1000])
        with pytest.raises(ValueError, match="must stay below 2\\^62"):
            fn(a, a, [2 ** 31] * 3)


# ---- the command-line tool -----------------------------------------------------------------------------
def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _cli(cohort_root, out, *args):
    r = run_bin("img_processing_parallel", "--mode", "3d", "--cpu", "--quiet", *args, "--data-root", cohort_root, "--out",
                str(out), "--json", str(out) + ".json")
    assert r.returncode == 0, r.stderr
    return tree(out)


@pytest.fixture(scope="module")
def cpu_trees(cohort_root, tmp_path_factory):
    base = tmp_path_factory.mktemp("vcmpcpu")
    plain = _cli(cohort_root, base / "plain")
    cube = _cli(cohort_root, base / "cube", "--volume-mask")  # the reference tree: the default 7 x 7 x 7 cube
    flagged = _cli(cohort_root, base / "flagged", "--dilate-mm", "2.5", "--volume-mask", "--compare-to", str(base / "cube"))
    return {"base": base, "plain": plain, "cube": cube, "flagged": flagged}


def test_cli_flagless_tree_unchanged_and_mask_round_trip(native, cohort_root, cpu_trees):
    from nm03_capstone_project_amd.utils import read_volume_mask
    plain, cube = cpu_trees["plain"], cpu_trees["cube"]
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    # a run without the flags writes the planes alone; --volume-mask adds two files per patient and changes no other
    assert all(k.endswith(("_original.jpg", "_processed.jpg")) for k in plain)
    assert set(cube) - set(plain) == {os.path.join(p, f) for p in pids for f in ("mask.mhd", "mask.raw")}
    assert all(cube[k] == plain[k] for k in plain)
    pj = json.load(open(str(cpu_trees["base"] / "plain") + ".json"))
    assert "compare" not in pj and "volume_mask" not in pj and all("compare_s" not in p for p in pj["patients"])
    assert json.load(open(str(cpu_trees["base"] / "cube") + ".json"))["volume_mask"] == {"patients": len(pids)}
    for pid in pids:
        mask, spacing = read_volume_mask(str(cpu_trees["base"] / "cube" / pid))
        arr, sp = native.mhd_read(str(cpu_trees["base"] / "cube" / pid / "mask.mhd"))
        assert arr.dtype == np.uint8 and set(np.unique(arr)) <= {0, 1} and np.array_equal(arr, mask) and mask.any()
        assert "MET_UCHAR" in cube[os.path.join(pid, "mask.mhd")].decode()
        assert len(cube[os.path.join(pid, "mask.raw")]) == mask.size
        assert len(spacing) == 3 and all(v > 0 for v in spacing)


def test_cli_cpu_compare_tree(native, cohort_root, cpu_trees):
    from nm03_capstone_project_amd.utils import read_volume_comparisons, read_volume_mask
    flagged, cube, base = cpu_trees["flagged"], cpu_trees["cube"], cpu_trees["base"]
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    assert set(flagged) - set(cube) == {"comparisons.csv"} | {os.path.join(p, "compare.json") for p in pids}
    rows = read_volume_comparisons(str(base / "flagged"))
    assert [r["patient"] for r in rows] == pids and all(r["status"] == "ok" for r in rows)
    assert flagged["comparisons.csv"].decode().splitlines()[0] == native.volume_compare_csv_header()
    dice, hd = [], 0.0
    for pid, row in zip(pids, rows):
        text = flagged[os.path.join(pid, "compare.json")].decode()
        js = json.loads(text)
        assert tuple(js) == cc.JSON_KEYS and js["reference"] == os.path.join(str(base / "cube"), pid, "mask.mhd")
        a, spacing = read_volume_mask(str(base / "flagged" / pid))
        b, _ = read_volume_mask(str(base / "cube" / pid))
        um = list(native.volume_spacing_um(*spacing))
        assert js["compare_spacing_um"] == um
        g = native.golden_compare_volumes(a, b, um)
        d, h, w = a.shape
        assert text == native.volume_compare_to_json(g, w, h, d, um, js["reference"])
        assert g["a_vox"] != g["b_vox"] and g["tp_vox"] > 0  # a 2.5 mm margin against the cube: the masks differ and overlap
        assert g["found_ab"] and js["hausdorff_mm"] > 0 and 0 < js["dice"] < 1
        for k in cc.JSON_KEYS:
            if isinstance(js[k], list):
                assert [row[k + ax] for ax in ("_x", "_y", "_z")] == js[k]
            else:
                assert row[k] == js[k], k
        dice.append(js["dice"])
        hd = max(hd, js["hausdorff_mm"])
    run = json.load(open(str(base / "flagged") + ".json"))
    assert run["compare"]["volumes"] == len(pids) and run["compare"]["hausdorff_mm_max"] == hd
    assert run["compare"]["dice_mean"] == float("%.9g" % (sum(dice) / len(dice)))
    assert run["volume_mask"] == {"patients": len(pids)} and all("compare_s" in p for p in run["patients"])


def test_cli_cpu_two_ranks_same_tree(cohort_root, cpu_trees, tmp_path):
    two = _cli(cohort_root, tmp_path / "flagged", "--dilate-mm", "2.5", "--volume-mask", "--compare-to", str(cpu_trees["base"] / "cube"),
               "--gpus", "2")
    assert two == cpu_trees["flagged"]


def test_cli_composes_with_the_other_flags(cohort_root, cpu_trees, tmp_path):
    """The comparison files are the same whatever else is asked for, and nothing else changes for them."""
    ref = str(cpu_trees["base"] / "cube")
    more = ("--measure-volume", "--measure-volume-thickness", "--measure-volume-lesions", "2", "--volume-views", "--volume-mesh")
    with_cmp = _cli(cohort_root, tmp_path / "a", "--dilate-mm", "2.5", *more, "--volume-mask", "--compare-to", ref)
    without = _cli(cohort_root, tmp_path / "b", "--dilate-mm", "2.5", *more)
    assert all(with_cmp[k] == without[k] for k in without)
    extra = set(with_cmp) - set(without)
    assert all(k.endswith(("mask.mhd", "mask.raw", "compare.json")) or k == "comparisons.csv" for k in extra)
    assert all(with_cmp[k] == cpu_trees["flagged"][k] for k in extra)


def test_cli_no_reference_and_shape_mismatch(native, cohort_root, cpu_trees, tmp_path):
    from nm03_capstone_project_amd.utils import read_volume_comparisons
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    assert len(pids) >= 3
    ref = tmp_path / "ref"
    shutil.copytree(str(cpu_trees["base"] / "cube"), str(ref))
    shutil.rmtree(str(ref / pids[0]))  # no file
    arr, sp = native.mhd_read(str(ref / pids[1] / "mask.mhd"))
    native.mhd_write(str(ref / pids[1] / "mask"), np.ascontiguousarray(arr[:, :, :-1]), *[float(v) for v in sp])  # another shape
    arr2, sp2 = native.mhd_read(str(ref / pids[2] / "mask.mhd"))
    native.mhd_write(str(ref / pids[2] / "mask"), (arr2.astype(np.uint16) * 700), *[float(v) for v in sp2])  # non-zero means set
    out = tmp_path / "out"
    got = _cli(cohort_root, out, "--compare-to", str(ref))
    rows = read_volume_comparisons(str(out))
    assert [r["status"] for r in rows[:3]] == ["no_reference", "shape_mismatch", "ok"]
    for r in rows[:2]:
        assert all(v is None for k, v in r.items() if k not in ("patient", "status"))
        assert os.path.join(r["patient"], "compare.json") not in got
    # the run's own mask is the cube, so against the cube reference it is a perfect match, whatever the element type
    assert rows[2]["dice"] == 1.0 and rows[2]["hausdorff_mm"] == 0.0 and rows[2]["fp_vox"] == rows[2]["fn_vox"] == 0
    lines = got["comparisons.csv"].decode().splitlines()
    assert all(ln.count(",") == lines[0].count(",") for ln in lines[1:3])
    run = json.load(open(str(out) + ".json"))
    assert all(p["ok"] for p in run["patients"])  # neither status fails the patient
    assert run["compare"]["volumes"] == len(pids) - 2
    # every plane is what a run without the flag writes
    assert all(got[k] == v for k, v in cpu_trees["plain"].items())


@pytest.mark.parametrize("args,word", [
    (("--volume-mask",), "--volume-mask needs --mode 3d"),
    (("--compare-to", "REF"), "--compare-to needs --mode 3d"),
    (("--mode", "3d", "--volume-mask", "--split-volume"), "--volume-mask is not available with --split-volume"),
    (("--mode", "3d", "--compare-to", "REF", "--split-volume"), "--compare-to is not available with --split-volume"),
    (("--mode", "3d", "--compare-to", ""), "--compare-to needs a directory"),
    (("--mode", "3d", "--compare-to", "OUT"), "is the output directory"),
    (("--mode", "3d", "--compare-to", "OUT/../o/."), "is the output directory"),
])
def test_cli_rejections(cohort_root, tmp_path, args, word):
    out = tmp_path / "o"
    args = [str(tmp_path / "ref") if a == "REF" else a.replace("OUT", str(out)) for a in args]
    r = run_bin("img_processing_parallel", "--cpu", "--data-root", cohort_root, "--out", str(out), *args)
    assert r.returncode == 2 and word in r.stderr, r.stderr
    assert "--compare-to" in r.stderr or "--volume-mask" in r.stderr  # the message names the flag
    assert not out.exists()


def test_flags_in_help_and_bench():
    r = run_bin("img_processing_parallel", "--help")
    assert r.returncode == 0 and "--volume-mask" in r.stdout and "--compare-to DIR" in r.stdout
    r = run_bin("nm03_bench", "--config", "cohort", "--compare")
    assert r.returncode == 2 and "--compare needs --config volume and the GPU (not --host-only)" in r.stderr
    r = run_bin("nm03_bench", "--config", "volume", "--host-only", "--compare")
    assert r.returncode == 2 and "--compare needs --config volume and the GPU (not --host-only)" in r.stderr


def test_pipeline_refuses_host_only_and_bad_reference():
    import nm03_capstone_project_amd as nm
    with pytest.raises(ValueError, match="not available with host_only"):
        nm.VolumePipeline(nm.PipelineConfig(host_only=True), compare_to=np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="must be \\[D, H, W\\]"):
        nm.VolumePipeline(nm.PipelineConfig(), compare_to=np.zeros((3, 4), np.uint8))


def test_example_flag_needs_dilate_mm(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "volume_3d.py"), "--series", str(tmp_path), "--compare-to-cube"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--compare-to-cube needs --dilate-mm R" in r.stderr
