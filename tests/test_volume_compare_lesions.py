"""The lesion-wise comparison (nm03/volume_compare_lesions.h, --compare-lesions) on the CPU, everything compared with ==:
golden model == SciPy reference == the host run of K18's word logic on every case of volume_compare_lesion_cases at
N = 1, 2, 64 and both connectivities, both orders of the masks and with the bits past the width set; the worked
examples literally; Σ table == K17's tp_vox; totals and reported lesions == K8's / K10's golden models; the sidecar
text and its key order; both CSVs; the --cpu CLI at one and two ranks; no_reference / shape_mismatch rows; every refusal;
the flagless tree."""
import json
import os
import shutil

import numpy as np
import pytest

import volume_compare_lesion_cases as lc
import volume_compare_cases as cc
from conftest import run_bin

CASES = lc.cases()
UM = [1000, 1000, 1000]


@pytest.fixture(scope="module")
def golden(native):
    """The golden record of every case, N and connectivity, computed once."""
    return {(c["name"], n, conn): lc.plain(native.golden_compare_volume_lesions(c["a"], c["b"], n, conn))
            for c in CASES for n in lc.NS for conn in (6, 26)}


@pytest.mark.parametrize("c", CASES, ids=lc.ids(CASES))
def test_golden_equals_reference_equals_words(native, golden, c):
    from nm03_capstone_project_amd.ops import reference
    for n in lc.NS:
        for conn in (6, 26):
            g = golden[(c["name"], n, conn)]
            assert tuple(g) == lc.DICT_KEYS and g["connectivity"] == conn and g["max_lesions"] == n
            assert all(tuple(r) == lc.RECORD_KEYS for r in g["a_lesions"] + g["b_lesions"])
            assert lc.plain(reference.compare_volume_lesions(c["a"], c["b"], n, conn)) == g
            assert lc.plain(native.volume_compare_lesions_words(c["a"], c["b"], n, conn)) == g
            assert lc.plain(native.volume_compare_lesions_words(c["a"], c["b"], n, conn, junk=True)) == g
            # the swap exchanges the sides and transposes the table
            assert lc.plain(native.golden_compare_volume_lesions(c["b"], c["a"], n, conn)) == lc.swapped(g)
            assert lc.plain(native.volume_compare_lesions_words(c["b"], c["a"], n, conn, junk=True)) == lc.swapped(g)
            assert (g["lesions_a"], g["lesions_b"]) == (c["counts"][0:2] if conn == 6 else c["counts"][2:4])
            assert len(g["a_lesions"]) == min(n, g["lesions_a"]) and len(g["b_lesions"]) == min(n, g["lesions_b"])


@pytest.mark.parametrize("c", CASES, ids=lc.ids(CASES))
def test_consistency_with_k17_k8_k10(native, golden, c):
    """Σ table == tp_vox; totals == the components of golden_measure_volume; the reported lesions' voxels and first ==
    golden_measure_volume_lesions of the same mask; a record's overlap is its row / column sum."""
    tp = native.golden_compare_volumes(c["a"], c["b"], UM)["tp_vox"]
    raw = np.zeros(c["a"].shape, np.uint16)
    for conn in (6, 26):
        for n in lc.NS:
            g = golden[(c["name"], n, conn)]
            t = np.asarray(g["table"], dtype=np.int64)
            assert int(t.sum()) == tp
            for tag, mask, line in (("a", c["a"], t.sum(axis=1)), ("b", c["b"], t.sum(axis=0))):
                vm = native.golden_measure_volume(np.array(mask), np.array(mask), raw, connectivity=conn)
                assert g["lesions_" + tag] == vm["components"]
                recs = g[tag + "_lesions"]
                k10 = native.golden_measure_volume_lesions(np.array(mask), raw, n, connectivity=conn)
                assert [(r["voxels"], r["first"]) for r in recs] == [(l["voxels"], list(l["first"])) for l in k10]
                assert [r["overlap_vox"] for r in recs] == [int(v) for v in line[:len(recs)]]
                assert g["hit_" + tag] >= sum(r["overlap_vox"] > 0 for r in recs)
                assert all(r["multi"] in (0, 1) and (r["best"] == -1) == (r["partners_reported"] == 0) for r in recs)
            if n == lc.MAX_LESIONS and not c["exceeds"]:
                assert t[n].sum() == 0 and t[:, n].sum() == 0


def test_worked_example_boxes(native, golden):
    for n in lc.NS:
        g = golden[("worked_boxes", n, 26)]
        assert {k: g[k] for k in lc.TOTAL_KEYS} == {"lesions_a": 1, "hit_a": 1, "multi_a": 0, "lesions_b": 2, "hit_b": 1, "multi_b": 0}
    g = golden[("worked_boxes", 2, 26)]
    assert g["table"] == [[48, 0, 0], [0, 0, 0], [0, 0, 0]]
    js = json.loads(native.volume_compare_to_json(native.golden_compare_volumes(lc.case("worked_boxes")["a"], lc.case("worked_boxes")["b"], UM),
                                                  16, 8, 5, UM, "", g))
    assert js["lesion_sensitivity"] == 0.5 and js["lesion_precision"] == 1 and js["lesion_f1"] == float("%.9g" % (2 / 3))


def test_worked_example_row(native, golden):
    g = golden[("worked_row", 2, 6)]
    assert {k: g[k] for k in lc.TOTAL_KEYS} == {"lesions_a": 3, "hit_a": 2, "multi_a": 0, "lesions_b": 2, "hit_b": 1, "multi_b": 1}
    assert g["b_lesions"][0] == {"voxels": 3, "first": [2, 0, 0], "overlap_vox": 2, "partners_reported": 2, "overlap_other_vox": 0,
                                 "multi": 1, "best": 0, "best_overlap_vox": 1}
    assert g["b_lesions"][1]["overlap_vox"] == 0 and g["b_lesions"][1]["best"] == -1 and g["b_lesions"][1]["first"] == [11, 0, 0]
    c = lc.case("worked_row")
    js = json.loads(native.volume_compare_to_json(native.golden_compare_volumes(c["a"], c["b"], UM), 12, 1, 1, UM, "", g))
    assert js["lesion_sensitivity"] == 0.5 and js["lesion_precision"] == float("%.9g" % (2 / 3)) and js["lesion_f1"] == 0.5
    assert js["b_lesions"][0]["best_dice"] == float("%.9g" % (1 / 3)) and js["b_lesions"][1]["best_dice"] is None
    assert js["b_lesions"][0]["coverage"] == float("%.9g" % (2 / 3)) and js["b_lesions"][1]["coverage"] == 0
    g1 = golden[("worked_row", 1, 6)]
    b0 = g1["b_lesions"][0]
    assert (b0["partners_reported"], b0["overlap_other_vox"], b0["multi"]) == (1, 1, 1)
    g64 = golden[("worked_row", 64, 6)]
    assert len(g64["a_lesions"]) == 3 and [r["first"] for r in g64["a_lesions"]] == [[0, 0, 0], [4, 0, 0], [9, 0, 0]]


def test_special_cases(golden):
    g = golden[("merge", 64, 26)]
    assert (g["multi_a"], g["multi_b"], g["hit_a"], g["hit_b"]) == (1, 0, 1, 3) and g["a_lesions"][0]["partners_reported"] == 3
    g = golden[("split", 64, 26)]
    assert (g["multi_a"], g["multi_b"], g["hit_a"], g["hit_b"]) == (0, 1, 3, 1) and g["b_lesions"][0]["partners_reported"] == 3
    g = golden[("touch_one", 2, 26)]
    assert g["a_lesions"][0]["overlap_vox"] == g["b_lesions"][0]["overlap_vox"] == 1 and g["hit_a"] == g["hit_b"] == 1
    g = golden[("best_tie", 2, 26)]
    b0 = g["b_lesions"][0]
    assert b0["partners_reported"] == 2 and b0["best"] == 0 and b0["best_overlap_vox"] == 2 and g["table"][0][0] == g["table"][1][0] == 2
    g = golden[("equal_areas", 64, 26)]  # equal areas: the earlier first voxel (z, y, x) first
    assert [r["first"] for r in g["a_lesions"]] == [[10, 0, 0], [30, 3, 1], [60, 5, 3]]
    g6, g26 = golden[("diagonal", 64, 6)], golden[("diagonal", 64, 26)]
    assert (g6["lesions_a"], g6["lesions_b"], g26["lesions_a"], g26["lesions_b"]) == (3, 4, 2, 2)
    g = golden[("lattice", 64, 26)]
    t = np.asarray(g["table"])
    assert t[64, :64].sum() > 0 and t[:64, 64].sum() > 0 and t[64, 64] == 5
    assert g["a_lesions"][0]["overlap_other_vox"] > 0 and g["b_lesions"][0]["overlap_other_vox"] > 0
    for name in ("a_empty", "b_empty", "both_empty"):
        g = golden[(name, 64, 26)]
        assert g["hit_a"] == g["hit_b"] == g["multi_a"] == g["multi_b"] == 0 and not np.asarray(g["table"]).any()
    g = golden[("equal", 64, 6)]  # A == B: every lesion hit by exactly its twin
    assert g["hit_a"] == g["lesions_a"] == g["hit_b"] == g["lesions_b"] and g["multi_a"] == g["multi_b"] == 0
    assert all(r["best"] == i and r["best_overlap_vox"] == r["voxels"] for i, r in enumerate(g["a_lesions"]))
    g = golden[("subset", 64, 26)]  # A ⊂ B: every lesion of A is covered entirely
    assert g["hit_a"] == g["lesions_a"] and all(r["overlap_vox"] == r["voxels"] for r in g["a_lesions"])


# ---- the writers ---------------------------------------------------------------------------------------------
def _floats(v):
    return None if v is None else float("%.9g" % v)


def test_sidecar_text_and_key_order(native, golden):
    for name, n, conn in (("worked_row", 2, 6), ("lattice", 64, 26), ("both_empty", 1, 26), ("size", 2, 26)):
        c = lc.case(name)
        d, h, w = c["a"].shape
        g = golden[(name, n, conn)]
        k17 = native.golden_compare_volumes(c["a"], c["b"], UM)
        short = native.volume_compare_to_json(k17, w, h, d, UM, "ref")
        text = native.volume_compare_to_json(k17, w, h, d, UM, "ref", g)
        assert native.volume_compare_to_json(k17, w, h, d, UM, "ref", None) == short
        js = json.loads(text)
        assert tuple(js) == cc.JSON_KEYS + lc.JSON_LESION_KEYS
        # removing the new keys gives the old text byte for byte: the new keys are one insertion before the closing brace
        cut = text.index(',"lesions_connectivity"')
        assert text[:cut] + "}\n" == short and text.endswith("}\n")
        assert js["lesions_connectivity"] == conn and js["lesions_max"] == n
        for k in lc.TOTAL_KEYS:
            assert js[k] == g[k]
        la, ha, lb, hb = g["lesions_a"], g["hit_a"], g["lesions_b"], g["hit_b"]
        assert js["lesion_sensitivity"] == _floats(hb / lb if lb else None)
        assert js["lesion_precision"] == _floats(ha / la if la else None)
        den = 2 * hb + (la - ha) + (lb - hb)
        assert js["lesion_f1"] == _floats(2 * hb / den if den else None)
        for tag, other in (("a", "b"), ("b", "a")):
            assert len(js[tag + "_lesions"]) == len(g[tag + "_lesions"])
            for rj, rg in zip(js[tag + "_lesions"], g[tag + "_lesions"]):
                assert tuple(rj) == lc.JSON_RECORD_KEYS and {k: rj[k] for k in lc.RECORD_KEYS} == rg
                assert rj["coverage"] == _floats(rg["overlap_vox"] / rg["voxels"])
                partner = g[other + "_lesions"][rg["best"]]["voxels"] if rg["best"] >= 0 else None
                assert rj["best_dice"] == _floats(None if partner is None else 2 * rg["best_overlap_vox"] / (rg["voxels"] + partner))


def test_csv_writers(native, golden):
    c = lc.case("lattice")
    d, h, w = c["a"].shape
    g = golden[("lattice", 2, 26)]
    k17 = native.golden_compare_volumes(c["a"], c["b"], UM)
    head, head_l = native.volume_compare_csv_header(), native.volume_compare_csv_header(True)
    assert native.volume_compare_csv_header(False) == head and head_l == head + "," + ",".join(lc.CSV_LESION_COLUMNS)
    short = native.volume_compare_csv_fields(k17, w, h, d, UM, "ref")
    full = native.volume_compare_csv_fields(k17, w, h, d, UM, "ref", g)
    assert full.startswith(short + ",") and ("patient,status," + full).count(",") == head_l.count(",")
    js = json.loads(native.volume_compare_to_json(k17, w, h, d, UM, "ref", g))
    assert full[len(short) + 1:].split(",") == [str(g[k]) for k in lc.TOTAL_KEYS] + [
        "%.9g" % js[k] for k in ("lesion_sensitivity", "lesion_precision", "lesion_f1")]
    e = golden[("both_empty", 2, 26)]  # null is an empty field
    ke = native.golden_compare_volumes(lc.case("both_empty")["a"], lc.case("both_empty")["b"], UM)
    assert native.volume_compare_csv_fields(ke, 70, 6, 4, UM, "", e).endswith(",0,0,0,0,0,0,,,")
    assert native.volume_compare_lesions_table_header() == ",".join(lc.TABLE_COLUMNS)
    rows = native.volume_compare_lesions_table_rows("P1", g).splitlines()
    assert len(rows) == 4 and [r.split(",")[:3] for r in rows] == [["P1", "a", "0"], ["P1", "a", "1"], ["P1", "b", "0"], ["P1", "b", "1"]]
    r0 = g["a_lesions"][0]
    assert rows[0].split(",")[3:] == [str(v) for v in (r0["voxels"], *r0["first"], r0["overlap_vox"], r0["partners_reported"],
                                                        r0["overlap_other_vox"], r0["multi"], r0["best"], r0["best_overlap_vox"])]


def test_bindings_refuse_bad_arguments(native):
    a = np.zeros((2, 3, 4), np.uint8)
    for fn in (native.golden_compare_volume_lesions, native.volume_compare_lesions_words):
        with pytest.raises(ValueError):
            fn(a, np.zeros((2, 3, 5), np.uint8), 2)
        with pytest.raises(ValueError):
            fn(a[0], a[0], 2)
        for n in (0, 65, -1):
            with pytest.raises(ValueError, match="max_lesions must be 1..64"):
                fn(a, a, n)
        with pytest.raises(ValueError, match="connectivity must be 6 or 26"):
            fn(a, a, 2, 18)
    from nm03_capstone_project_amd.ops import reference
    with pytest.raises(ValueError):
        reference.compare_volume_lesions(a, a, 0)
    with pytest.raises(ValueError):
        reference.compare_volume_lesions(a, a, 2, 18)


def test_pipeline_argument_checks():
    import nm03_capstone_project_amd as nm
    ref = np.zeros((2, 3, 4), np.uint8)
    with pytest.raises(ValueError, match="compare_lesions needs compare_to"):
        nm.VolumePipeline(nm.PipelineConfig(), compare_lesions=2)
    for n in (-1, 65):
        with pytest.raises(ValueError, match="compare_lesions must be 0 \\(off\\) or 1..64"):
            nm.VolumePipeline(nm.PipelineConfig(), compare_to=ref, compare_lesions=n)
    assert nm.VolumePipeline(nm.PipelineConfig(), compare_to=ref, compare_lesions=64).compare_lesions == 64


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


N_CLI = 3


@pytest.fixture(scope="module")
def cpu_trees(cohort_root, tmp_path_factory):
    base = tmp_path_factory.mktemp("vclcpu")
    plain = _cli(cohort_root, base / "plain")
    cube = _cli(cohort_root, base / "cube", "--volume-mask")  # the reference tree: the default 7 x 7 x 7 cube
    flags = ("--dilate-mm", "2.5", "--volume-mask", "--compare-to", str(base / "cube"))
    compared = _cli(cohort_root, base / "compared", *flags)
    flagged = _cli(cohort_root, base / "flagged", *flags, "--compare-lesions", str(N_CLI))
    return {"base": base, "plain": plain, "cube": cube, "compared": compared, "flagged": flagged, "flags": flags}


def test_cli_cpu_tree(native, cohort_root, cpu_trees):
    from nm03_capstone_project_amd.utils import read_volume_comparisons, read_volume_lesion_comparisons, read_volume_mask
    flagged, compared, base = cpu_trees["flagged"], cpu_trees["compared"], cpu_trees["base"]
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    # the flag adds one file and changes compare.json and comparisons.csv; every other file is what --compare-to alone writes
    assert set(flagged) - set(compared) == {"compare_lesions.csv"}
    changed = {k for k in compared if flagged[k] != compared[k]}
    assert changed == {"comparisons.csv"} | {os.path.join(p, "compare.json") for p in pids}
    rows = read_volume_comparisons(str(base / "flagged"))
    old_rows = read_volume_comparisons(str(base / "compared"))
    lines = flagged["comparisons.csv"].decode().splitlines()
    old_lines = compared["comparisons.csv"].decode().splitlines()
    assert lines[0] == native.volume_compare_csv_header(True) and old_lines[0] == native.volume_compare_csv_header()
    table = read_volume_lesion_comparisons(str(base / "flagged"))
    assert flagged["compare_lesions.csv"].decode().splitlines()[0] == ",".join(lc.TABLE_COLUMNS)
    want_table, f1 = [], []
    for pid, row, old_row, line, old_line in zip(pids, rows, old_rows, lines[1:], old_lines[1:]):
        text = flagged[os.path.join(pid, "compare.json")].decode()
        js = json.loads(text)
        assert tuple(js) == cc.JSON_KEYS + lc.JSON_LESION_KEYS
        old = compared[os.path.join(pid, "compare.json")].decode()
        assert text[:text.index(',"lesions_connectivity"')] + "}\n" == old  # removing the new keys gives the old text
        assert line.startswith(old_line + ",") and {k: row[k] for k in old_row} == old_row
        a, spacing = read_volume_mask(str(base / "flagged" / pid))
        b, _ = read_volume_mask(str(base / "cube" / pid))
        um = list(native.volume_spacing_um(*spacing))
        g = native.golden_compare_volume_lesions(a, b, N_CLI, 26)
        d, h, w = a.shape
        assert text == native.volume_compare_to_json(native.golden_compare_volumes(a, b, um), w, h, d, um, js["reference"], g)
        assert js["lesions_connectivity"] == 26 and js["lesions_max"] == N_CLI and js["hit_b"] >= 1 and js["lesions_a"] >= 1
        for k in lc.CSV_LESION_COLUMNS:
            assert row[k] == js[k], k
        for tag in ("a", "b"):
            for i, r in enumerate(g[tag + "_lesions"]):
                want_table.append({"patient": pid, "side": tag, "lesion": i, "voxels": r["voxels"], "first_x": r["first"][0],
                                   "first_y": r["first"][1], "first_z": r["first"][2],
                                   **{k: r[k] for k in lc.RECORD_KEYS if k not in ("voxels", "first")}})
        if js["lesion_f1"] is not None:
            f1.append(js["lesion_f1"])
    assert table == want_table and all(tuple(r) == lc.TABLE_COLUMNS for r in table)
    run = json.load(open(str(base / "flagged") + ".json"))
    old_run = json.load(open(str(base / "compared") + ".json"))
    assert run["compare"]["lesions"] is True and run["compare"]["lesion_f1_mean"] == float("%.9g" % (sum(f1) / len(f1)))
    assert {k: v for k, v in run["compare"].items() if k not in ("lesions", "lesion_f1_mean")} == old_run["compare"]
    assert "lesions" not in old_run["compare"] and all("compare_lesions_s" in p for p in run["patients"])
    assert all("compare_lesions_s" not in p for p in old_run["patients"])


def test_cli_cpu_two_ranks_same_tree(cohort_root, cpu_trees, tmp_path):
    two = _cli(cohort_root, tmp_path / "flagged", *cpu_trees["flags"], "--compare-lesions", str(N_CLI), "--gpus", "2")
    assert two == cpu_trees["flagged"]


def test_cli_connectivity_and_composition(native, cohort_root, cpu_trees, tmp_path):
    """--measure-volume-connectivity 6 is the lesions' connectivity; the lesion files are the same whatever else is asked for."""
    more = ("--measure-volume", "--measure-volume-thickness", "--measure-volume-lesions", "2", "--volume-views", "--volume-mesh")
    six = _cli(cohort_root, tmp_path / "six", *cpu_trees["flags"], "--compare-lesions", str(N_CLI), "--measure-volume-connectivity", "6")
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    assert all(json.loads(six[os.path.join(p, "compare.json")])["lesions_connectivity"] == 6 for p in pids)
    with_more = _cli(cohort_root, tmp_path / "more", *cpu_trees["flags"], "--compare-lesions", str(N_CLI), *more)
    without = _cli(cohort_root, tmp_path / "without", "--dilate-mm", "2.5", *more)
    assert all(with_more[k] == without[k] for k in without)
    extra = set(with_more) - set(without)
    assert "compare_lesions.csv" in extra and all(with_more[k] == cpu_trees["flagged"][k] for k in extra)


def test_cli_no_reference_and_shape_mismatch(native, cohort_root, cpu_trees, tmp_path):
    from nm03_capstone_project_amd.utils import read_volume_comparisons, read_volume_lesion_comparisons
    pids = native.find_patient_dirs(native.cohort_dir(cohort_root))
    assert len(pids) >= 3
    ref = tmp_path / "ref"
    shutil.copytree(str(cpu_trees["base"] / "cube"), str(ref))
    shutil.rmtree(str(ref / pids[0]))  # no file
    arr, sp = native.mhd_read(str(ref / pids[1] / "mask.mhd"))
    native.mhd_write(str(ref / pids[1] / "mask"), np.ascontiguousarray(arr[:, :, :-1]), *[float(v) for v in sp])  # another shape
    out = tmp_path / "out"
    got = _cli(cohort_root, out, "--compare-to", str(ref), "--compare-lesions", "2")
    rows = read_volume_comparisons(str(out))
    assert [r["status"] for r in rows[:3]] == ["no_reference", "shape_mismatch", "ok"]
    for r in rows[:2]:
        assert all(v is None for k, v in r.items() if k not in ("patient", "status")) and set(lc.CSV_LESION_COLUMNS) <= set(r)
    lines = got["comparisons.csv"].decode().splitlines()
    assert all(ln.count(",") == lines[0].count(",") for ln in lines[1:])
    # the run's own mask is the cube: against the cube every lesion is hit by its twin
    assert rows[2]["lesion_f1"] == 1.0 and rows[2]["hit_a"] == rows[2]["lesions_a"] == rows[2]["lesions_b"] and rows[2]["multi_a"] == 0
    table = read_volume_lesion_comparisons(str(out))
    assert table and {r["patient"] for r in table} == set(pids[2:])
    run = json.load(open(str(out) + ".json"))
    assert all(p["ok"] for p in run["patients"]) and run["compare"]["lesion_f1_mean"] == 1
    assert all(got[k] == v for k, v in cpu_trees["plain"].items())


def test_cli_flagless_tree_unchanged(cpu_trees):
    plain, compared = cpu_trees["plain"], cpu_trees["compared"]
    assert all(k.endswith(("_original.jpg", "_processed.jpg")) for k in plain)
    assert "compare_lesions.csv" not in compared and b"lesion" not in compared["comparisons.csv"]
    pj = json.load(open(str(cpu_trees["base"] / "plain") + ".json"))
    assert "compare" not in pj and all("compare_lesions_s" not in p for p in pj["patients"])


@pytest.mark.parametrize("args,word", [
    (("--mode", "3d", "--compare-lesions", "2"), "--compare-lesions needs --compare-to DIR"),
    (("--compare-to", "REF", "--compare-lesions", "2"), "--compare-lesions needs --mode 3d"),
    (("--mode", "3d", "--compare-to", "REF", "--compare-lesions", "2", "--split-volume"), "--compare-lesions is not available with --split-volume"),
    (("--mode", "3d", "--compare-to", "REF", "--compare-lesions", "0"), "--compare-lesions must be an integer from 1 to 64"),
    (("--mode", "3d", "--compare-to", "REF", "--compare-lesions", "65"), "--compare-lesions must be an integer from 1 to 64"),
    (("--mode", "3d", "--compare-to", "REF", "--compare-lesions", "two"), "--compare-lesions must be an integer from 1 to 64"),
])
def test_cli_rejections(cohort_root, tmp_path, args, word):
    out = tmp_path / "o"
    args = [str(tmp_path / "ref") if a == "REF" else a for a in args]
    r = run_bin("img_processing_parallel", "--cpu", "--data-root", cohort_root, "--out", str(out), *args)
    assert r.returncode == 2 and word in r.stderr, r.stderr
    assert not out.exists()


def test_flag_in_help_and_bench():
    r = run_bin("img_processing_parallel", "--help")
    assert r.returncode == 0 and "--compare-lesions N" in r.stdout
    r = run_bin("nm03_bench", "--config", "volume", "--compare-lesions", "8")
    assert r.returncode == 2 and "--compare-lesions needs --compare" in r.stderr
    r = run_bin("nm03_bench", "--config", "volume", "--compare", "--compare-lesions", "65")
    assert r.returncode == 2 and "--compare-lesions must be 1..64" in r.stderr
