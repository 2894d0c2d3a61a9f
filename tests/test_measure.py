"""--measure on the CPU: the golden model against an independent SciPy reference on every named mask,
analytic cases, the Euler identity of the shared bit-quad function, the sidecar text, and the cohort
CLI's files (sidecars, measurements.csv, --gpus 2, --resume, flag validation)."""
import json
import os

import numpy as np
import pytest

import measure_masks as mm
from conftest import run_bin

SHAPES = [(1, 1), (3, 5), (64, 64), (77, 131), (100, 100), (256, 256)]
KEYS = ["width", "height", "connectivity", "area_px", "region_px", "bbox", "sum_x", "sum_y", "perimeter_edges", "components",
        "largest_px", "holes", "raw_sum", "raw_min", "raw_max", "area_mm2", "centroid_x", "centroid_y", "centroid_x_mm",
        "centroid_y_mm", "mean"]


def golden(native, mask, conn, raw=None, pixel_type="u16", stored_bits=16):
    h, w = mask.shape
    raw = mm.raw_of(h, w) if raw is None else raw
    return native.golden_measure(mask.astype(np.uint8), mm.region_of(mask).astype(np.uint8), raw, pixel_type, stored_bits, conn)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_golden_equals_scipy_reference(native, shape, conn):
    from nm03_capstone_project_amd.ops import reference
    h, w = shape
    raw = mm.raw_of(h, w)
    for name in mm.NAMES:
        mask = mm.build(name, h, w)
        want = reference.measure(mask, mm.region_of(mask), raw, conn)
        assert golden(native, mask, conn, raw) == want, name


@pytest.mark.parametrize("pixel_type,bits", [("i16", 16), ("u16", 12), ("i16", 12)])
def test_golden_intensities_by_type(native, pixel_type, bits):
    from nm03_capstone_project_amd.ops import reference
    mask = mm.build("ring", 64, 64)
    raw = mm.raw_of(64, 64, seed=3)
    got = golden(native, mask, 8, raw, pixel_type, bits)
    assert got == reference.measure(mask, mm.region_of(mask), raw, 8, pixel_type, bits)
    assert got["raw_min"] < got["raw_max"]
    if pixel_type == "i16":
        assert got["raw_min"] < 0
    else:
        assert 0 <= got["raw_min"] and got["raw_max"] < 1 << bits


def test_analytic_cases(native):
    cb = mm.build("checkerboard", 8, 8)
    assert golden(native, cb, 4)["components"] == 32 and golden(native, cb, 4)["largest_px"] == 1
    assert golden(native, cb, 8)["components"] == 1 and golden(native, cb, 8)["largest_px"] == 32
    for conn in (4, 8):
        assert golden(native, mm.build("ring", 64, 64), conn)["holes"] == 1
    n = 37
    d = golden(native, mm.build("diag", n, n), 4)
    assert d["components"] == n and d["perimeter_edges"] == 4 * n and d["holes"] == 0
    assert golden(native, mm.build("diag", n, n), 8)["components"] == 1
    e = golden(native, mm.build("empty", 20, 30), 8)
    assert e["bbox"] == [-1, -1, -1, -1]
    assert (e["area_px"], e["components"], e["holes"], e["raw_sum"], e["raw_min"], e["raw_max"]) == (0, 0, 0, 0, 0, 0)
    js = json.loads(native.measure_to_json(e, 30, 20))
    assert js["area_mm2"] == 0 and all(js[k] is None for k in KEYS[-5:])
    f = golden(native, mm.build("full", 20, 30), 8)
    assert (f["area_px"], f["bbox"], f["perimeter_edges"], f["components"], f["holes"]) == (600, [0, 0, 29, 19], 100, 1, 0)
    assert (f["sum_x"], f["sum_y"]) == (20 * sum(range(30)), 30 * sum(range(20)))


@pytest.mark.parametrize("conn", [4, 8])
def test_euler_identity(native, conn):
    """components − holes of the golden (flood fills, complement labelling) equals the bit-quad function the
    kernel uses, on every mask; the widths cover a full last word (64, 256) and partial ones."""
    for h, w in SHAPES + [(5, 128), (2, 65)]:
        for name in mm.NAMES:
            mask = mm.build(name, h, w)
            g = golden(native, mask, conn)
            assert g["components"] - g["holes"] == native.measure_euler(mask.astype(np.uint8), conn), (name, h, w)


def test_to_json_exact(native):
    rec = {"area_px": 14, "region_px": 9, "bbox": [1, 1, 5, 3], "sum_x": 42, "sum_y": 28, "perimeter_edges": 20,
           "components": 1, "largest_px": 14, "holes": 1, "raw_sum": -238, "raw_min": -80, "raw_max": 26}
    text = native.measure_to_json(rec, 7, 5, 0.5, 0.25, 2.0, -10.0, True, 8)
    assert text == ('{"width":7,"height":5,"connectivity":8,"area_px":14,"region_px":9,"bbox":[1,1,5,3],"sum_x":42,"sum_y":28,'
                    '"perimeter_edges":20,"components":1,"largest_px":14,"holes":1,"raw_sum":-238,"raw_min":-80,"raw_max":26,'
                    '"area_mm2":1.75,"centroid_x":3,"centroid_y":2,"centroid_x_mm":1.5,"centroid_y_mm":0.5,"mean":-44}\n')
    assert list(json.loads(text)) == KEYS
    # without the rescale the mean is the stored mean; nine significant digits
    rec["raw_sum"] = 100
    assert '"mean":7.14285714}' in native.measure_to_json(rec, 7, 5, 0.5, 0.25, 2.0, -10.0, False, 4)


# ---- CLI ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_cohort(tmp_path_factory, native):
    root = str(tmp_path_factory.mktemp("mdata")) + "/"
    native.synth_cohort(root, patients=2, min_slices=3, max_slices=3, threads=2)
    return root


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def cohort_files(native, root):
    base = native.cohort_dir(root)
    return [(pid, f) for pid in native.find_patient_dirs(base) for f in native.list_patient_series(base, pid)[1]]


@pytest.fixture(scope="module")
def cpu_run(small_cohort, tmp_path_factory):
    out = tmp_path_factory.mktemp("mcpu") / "out"
    r = run_bin("img_processing_parallel", "--cpu", "--measure", "--quiet", "--data-root", small_cohort, "--out", str(out),
                "--json", str(out) + ".json")
    assert r.returncode == 0, r.stderr
    return out


def test_cli_cpu_sidecars_and_table(native, small_cohort, cpu_run):
    import nm03_capstone_project_amd as nm
    from nm03_capstone_project_amd.utils import read_measurements
    files = cohort_files(native, small_cohort)
    assert len(files) == 6
    pipe = nm.SlicePipeline(nm.PipelineConfig(measure=True))
    for pid, f in files:
        raw, meta = native.read_slice(f, 0)
        stem = os.path.splitext(os.path.basename(f))[0]
        side = (cpu_run / pid / f"{stem}_measure.json").read_bytes().decode()
        g = pipe.golden(raw, meta)
        assert side == g["measure_json"]
        assert json.loads(side)["area_px"] == g["measure"]["area_px"]
    lines = (cpu_run / "measurements.csv").read_text().splitlines()
    assert lines[0].split(",")[:4] == ["patient", "file", "status", "width"]
    assert len(lines) == 1 + 6 + 2 and sum(",TOTAL," in ln for ln in lines) == 2
    rows = read_measurements(str(cpu_run))
    for pid in {p for p, _ in files}:
        mine = [r for r in rows if r["patient"] == pid and r["file"] != "TOTAL"]
        total = [r for r in rows if r["patient"] == pid and r["file"] == "TOTAL"]
        assert len(mine) == 3 and len(total) == 1 and all(r["status"] == "ok" for r in mine)
        assert total[0]["area_px"] == sum(r["area_px"] for r in mine)
        assert total[0]["area_mm2"] == pytest.approx(sum(r["area_mm2"] for r in mine), rel=1e-8)
    j = json.load(open(str(cpu_run) + ".json"))
    assert j["measure"]["slices"] == 6
    assert j["measure"]["area_px_total"] == sum(r["area_px"] for r in rows if r["file"] != "TOTAL")


def test_cli_cpu_two_ranks_identical(small_cohort, cpu_run, tmp_path):
    out = tmp_path / "out"
    r = run_bin("img_processing_parallel", "--cpu", "--measure", "--quiet", "--gpus", "2", "--data-root", small_cohort,
                "--out", str(out))
    assert r.returncode == 0, r.stderr
    assert tree(out) == tree(cpu_run)


def test_cli_cpu_resume_rewrites_only_the_missing_sidecar(native, small_cohort, cpu_run, tmp_path):
    import shutil
    out = tmp_path / "out"
    shutil.copytree(cpu_run, out)
    before = tree(out)
    sides = sorted(p for p in before if p.endswith("_measure.json"))
    victim = out / sides[2]
    victim.unlink()
    stamp = {p: os.stat(out / p).st_mtime_ns for p in before if p != sides[2] and p != "measurements.csv"}
    r = run_bin("img_processing_parallel", "--cpu", "--measure", "--quiet", "--resume", "--data-root", small_cohort, "--out",
                str(out))
    assert r.returncode == 0, r.stderr
    assert tree(out) == before
    # every slice but the victim was skipped (its JPEGs and sidecar untouched); the victim's JPEGs were rewritten with it
    stem = sides[2][:-len("_measure.json")]
    touched = {p for p, t in stamp.items() if os.stat(out / p).st_mtime_ns != t}
    assert touched <= {stem + "_original.jpg", stem + "_processed.jpg"}


def test_cli_without_flag_has_todays_files(native, small_cohort, tmp_path):
    out = tmp_path / "out"
    r = run_bin("img_processing_parallel", "--cpu", "--quiet", "--data-root", small_cohort, "--out", str(out))
    assert r.returncode == 0, r.stderr
    want = set()
    for pid, f in cohort_files(native, small_cohort):
        stem = os.path.splitext(os.path.basename(f))[0]
        want |= {f"{pid}/{stem}_original.jpg", f"{pid}/{stem}_processed.jpg"}
    assert set(tree(out)) == want


def test_test_pipeline_cpu_measure(native, cohort_root, tmp_path):
    import nm03_capstone_project_amd as nm
    plain, ms = tmp_path / "plain", tmp_path / "ms"
    assert run_bin("test_pipeline", "--cpu", "--data-root", cohort_root, "--out", str(plain)).returncode == 0
    r = run_bin("test_pipeline", "--cpu", "--measure", "--measure-connectivity", "4", "--data-root", cohort_root, "--out",
                str(ms))
    assert r.returncode == 0, r.stderr
    assert set(tree(ms)) == set(tree(plain)) | {"measure.json"}
    for name, data in tree(plain).items():
        assert tree(ms)[name] == data, name
    raw, meta = native.read_slice(native.test_slice_path(cohort_root), 0)
    g = nm.SlicePipeline(nm.PipelineConfig(measure=True, measure_connectivity=4)).golden(raw, meta)
    assert (ms / "measure.json").read_text() == g["measure_json"]
    assert json.loads(g["measure_json"])["connectivity"] == 4 and g["measure"]["area_px"] > 0


@pytest.mark.parametrize("tool", ["img_processing_parallel", "img_processing_sequential"])
def test_measure_rejects_3d_mode(tool, cohort_root, tmp_path):
    for args in (["--mode", "3d", "--measure"], ["--measure", "--mode", "3d"]):
        r = run_bin(tool, *args, "--data-root", cohort_root, "--out", str(tmp_path / "o"))
        assert r.returncode == 2 and "--measure is not available with --mode 3d" in r.stderr
        assert "unknown option" not in r.stderr and not (tmp_path / "o").exists()


@pytest.mark.parametrize("tool", ["test_pipeline", "img_processing_sequential", "img_processing_parallel"])
def test_measure_connectivity_rejects_6(tool, cohort_root, tmp_path):
    r = run_bin(tool, "--measure", "--measure-connectivity", "6", "--data-root", cohort_root, "--out", str(tmp_path / "o"))
    assert r.returncode == 2 and "--measure-connectivity must be 4 or 8" in r.stderr
    assert "unknown option" not in r.stderr and not (tmp_path / "o").exists()


def test_engine_rejects_measure_on_the_host_path(native):
    import nm03_capstone_project_amd as nm
    with pytest.raises(ValueError, match="measure"):
        native.Engine(nm.PipelineConfig(batch_size=1, streams=1, threads=1, measure=True, host_only=True).engine_config())


def test_measure_flags_in_help():
    r = run_bin("img_processing_parallel", "--help")
    assert r.returncode == 0 and "--measure " in r.stdout and "--measure-connectivity" in r.stdout
