"""--measure-intensity without a GPU: the golden model (sort), the NumPy reference (sort) and the host run
of the K11 kernels' two-pass radix select agree with `==` on every case; the rank formula, the sidecar
text and the standard deviation's exact radicand."""
import json
import math
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np
import pytest

from nm03_capstone_project_amd.ops import reference

import intensity_cases as ic

CASES_2D = ic.cases_2d()
CASES_3D = ic.cases_3d()


@pytest.mark.parametrize("name,mask,raw,ptype,bits", CASES_2D, ids=ic.ids(CASES_2D))
def test_golden_reference_and_words_agree_2d(native, name, mask, raw, ptype, bits):
    ref = reference.measure_intensity(mask, raw, ptype, bits)
    assert native.golden_measure_intensity(mask, raw, ptype, bits) == ref
    assert native.intensity_words(mask, raw, ptype, bits) == ref
    # set bits in the plane storage past the width must not count
    assert native.intensity_words(mask, raw, ptype, bits, stray_bits=True) == ref
    assert ref["count"] == int(mask.sum())


@pytest.mark.parametrize("name,mask,raw,ptype,bits", CASES_3D, ids=ic.ids(CASES_3D))
def test_golden_reference_and_words_agree_3d(native, name, mask, raw, ptype, bits):
    ref = reference.measure_volume_intensity(mask, raw, ptype, bits)
    assert native.golden_measure_volume_intensity(mask, raw, ptype, bits) == ref
    assert native.volume_intensity_words(mask, raw, ptype, bits) == ref


def test_cases_hit_what_they_are_built_for():
    by = {c[0]: c for c in CASES_2D}
    r = reference.measure_intensity(*by["clusters_2_2"][1:])
    assert (r["raw_p50"], r["raw_p75"]) == (0x10FF, 0x1100)
    assert reference.measure_intensity(*by["clusters_50_50"][1:])["raw_p50"] == 0x10FF
    assert reference.measure_intensity(*by["clusters_49_51"][1:])["raw_p50"] == 0x1100
    assert reference.measure_intensity(*by["clusters_25_75"][1:])["raw_p25"] == 0x10FF
    assert reference.measure_intensity(*by["i16_12_junk"][1:])["raw_p10"] < 0
    assert reference.measure_intensity(*by["i16_16"][1:])["raw_p10"] < 0 < reference.measure_intensity(*by["i16_16"][1:])["raw_p90"]
    assert reference.measure_intensity(*by["u16_high"][1:])["raw_p10"] >= 32768
    assert reference.measure_intensity(*by["full_512_65535"][1:])["raw_sum_sq"] == 512 * 512 * 65535 ** 2 > 2 ** 49
    assert reference.measure_intensity(*by["empty"][1:]) == {"count": 0, "raw_sum_sq": 0, **{f"raw_p{p}": 0 for p in ic.PERCENTILES}}
    m = by["256x300_second_trip"][1]
    assert m.shape[0] * ((m.shape[1] + 63) // 64) == 1200


def test_rank_formula_is_the_integer_ceiling(native):
    for n in range(0, 1001):
        for p in ic.PERCENTILES:
            k = native.intensity_rank(p, n)
            assert k == -((-p * n) // 100), (p, n)  # ceil(p · n / 100) in Python integers
            assert (1 <= k <= n) if n else k == 0
    # 64-bit: p · n does not wrap at the largest count a volume can have
    assert native.intensity_rank(90, 2 ** 32 - 1) == -((-90 * (2 ** 32 - 1)) // 100)


def _measure_record(native, mask, raw, ptype, bits):
    return native.golden_measure(mask.astype(np.uint8), mask.astype(np.uint8), raw, ptype, bits, 8)


def _check_appended(text, base, rec, st, slope, intercept, rescale):
    assert text.startswith(base[:-2] + ',"raw_sum_sq":') and text.endswith("}\n")
    obj = json.loads(text)
    keys = list(obj)
    assert keys[-13:] == list(ic.INT_KEYS + ic.DOUBLE_KEYS)
    assert keys[:-13] == list(json.loads(base))
    for k in ic.INT_KEYS:
        assert obj[k] == st[k]
    if st["count"] == 0:
        assert all(obj[k] is None for k in ic.DOUBLE_KEYS)
        return obj
    a, b = (slope, intercept) if rescale else (1.0, 0.0)
    for p, k in zip(ic.PERCENTILES, ("p10", "p25", "median", "p75", "p90")):
        assert obj[k] == pytest.approx(a * st[f"raw_p{p}"] + b, rel=1e-8, abs=1e-8)
    assert obj["iqr"] == pytest.approx(abs(a) * (st["raw_p75"] - st["raw_p25"]), rel=1e-8, abs=1e-6)
    n, s, q = st["count"], rec["raw_sum"], st["raw_sum_sq"]
    assert obj["std"] == pytest.approx(abs(a) * math.sqrt(Fraction(n * q - s * s, n * n)), rel=1e-8, abs=1e-8)
    return obj


@pytest.mark.parametrize("rescale,slope,intercept", [(True, 1.5, -1024.0), (True, -2.0, 100.0), (False, 3.0, 5.0)])
def test_sidecar_text_appends_the_keys_in_order_2d(native, rescale, slope, intercept):
    for name in ("70x5", "i16_16", "empty", "n1"):
        _, mask, raw, ptype, bits = next(c for c in CASES_2D if c[0] == name)
        h, w = mask.shape
        rec = _measure_record(native, mask, raw, ptype, bits)
        st = native.golden_measure_intensity(mask, raw, ptype, bits)
        base = native.measure_to_json(rec, w, h, 0.5, 0.75, slope, intercept, rescale, 8)
        text = native.measure_to_json(rec, w, h, 0.5, 0.75, slope, intercept, rescale, 8, intensity=st)
        obj = _check_appended(text, base, rec, st, slope, intercept, rescale)
        if rescale and slope < 0 and st["count"] > 1:
            assert obj["p10"] >= obj["p90"]  # the mapped raw order statistics
        dia = native.golden_measure_diameters(mask.astype(np.uint8), 8)
        base_d = native.measure_diameters_to_json(rec, dia, w, h, 0.5, 0.75, slope, intercept, rescale, 8)
        text_d = native.measure_diameters_to_json(rec, dia, w, h, 0.5, 0.75, slope, intercept, rescale, 8, intensity=st)
        _check_appended(text_d, base_d, rec, st, slope, intercept, rescale)
        assert base_d.startswith(base[:-2])


def test_sidecar_text_appends_the_keys_in_order_3d(native):
    for name in ("70x9x40_three_workgroups", "empty"):
        _, mask, raw, ptype, bits = next(c for c in CASES_3D if c[0] == name)
        d, h, w = mask.shape
        m8 = mask.astype(np.uint8)
        rec = native.golden_measure_volume(m8, m8, raw, ptype, bits, 26)
        st = native.golden_measure_volume_intensity(mask, raw, ptype, bits)
        args = (rec, w, h, d, 0.5, 0.75, 2.5, "position", 2.0, -7.0, True, 26)
        base = native.volume_measure_to_json(*args)
        _check_appended(native.volume_measure_to_json(*args, intensity=st), base, rec, st, 2.0, -7.0, True)
        lesions = native.golden_measure_volume_lesions(m8, raw, 2, ptype, bits, 26)
        with_l = native.volume_measure_to_json(*args, lesions=lesions, lesions_max=2)
        both = native.volume_measure_to_json(*args, lesions=lesions, lesions_max=2, intensity=st)
        # the new keys sit after `mean` and before lesions_max / lesions; everything else is unchanged
        head = base[:-2]
        assert with_l.startswith(head + ',"lesions_max":2,')
        keys = native.volume_measure_to_json(*args, intensity=st)[len(head):-2]
        assert both == head + keys + with_l[len(head):]
        assert list(json.loads(both))[-2:] == ["lesions_max", "lesions"]


def _exact_std(n, sum_sq, raw_sum):
    getcontext().prec = 60
    return (Decimal(n * sum_sq - raw_sum * raw_sum).sqrt() / Decimal(n))


def test_std_uses_the_exact_radicand(native):
    # 512 × 512 samples of 65535: the variance is exactly 0; Σv²/n − mean² in doubles is not
    _, mask, raw, ptype, bits = next(c for c in CASES_2D if c[0] == "full_512_65535")
    st = native.golden_measure_intensity(mask, raw, ptype, bits)
    n = st["count"]
    assert native.intensity_std(st, n * 65535) == 0.0
    # two values one apart near the top of the range: std = 0.5 exactly, lost by the double formula
    vals = np.array([65534, 65535] * 50000, np.int64)
    st2 = {"count": int(vals.size), "raw_sum_sq": int((vals * vals).sum()), **{f"raw_p{p}": 0 for p in ic.PERCENTILES}}
    got = native.intensity_std(st2, int(vals.sum()))
    exact = _exact_std(st2["count"], st2["raw_sum_sq"], int(vals.sum()))
    assert exact == Decimal("0.5")
    assert abs(Decimal(got) - exact) <= Decimal("1e-12") * exact
    # an uneven two-value mix, and a random case: 1e-12 relative against the exact value
    vals = np.array([3] * 7 + [65535] * 13, np.int64)
    st3 = {"count": 20, "raw_sum_sq": int((vals * vals).sum()), **{f"raw_p{p}": 0 for p in ic.PERCENTILES}}
    exact = _exact_std(20, st3["raw_sum_sq"], int(vals.sum()))
    assert abs(Decimal(native.intensity_std(st3, int(vals.sum()))) - exact) <= Decimal("1e-12") * exact
    _, mask, raw, ptype, bits = next(c for c in CASES_2D if c[0] == "256x300_second_trip")
    st4 = native.golden_measure_intensity(mask, raw, ptype, bits)
    s = int(raw[mask].astype(np.int64).sum())
    exact = _exact_std(st4["count"], st4["raw_sum_sq"], s)
    assert abs(Decimal(native.intensity_std(st4, s)) - exact) <= Decimal("1e-12") * exact
    assert native.intensity_std({"count": 0, "raw_sum_sq": 0, **{f"raw_p{p}": 0 for p in ic.PERCENTILES}}, 0) == 0.0


# ---- CLI (--cpu: the golden path) -----------------------------------------------------------------------
import os  # noqa: E402

from conftest import run_bin  # noqa: E402

NEW_COLUMNS = list(ic.INT_KEYS + ic.DOUBLE_KEYS)


@pytest.fixture(scope="module")
def small_cohort(tmp_path_factory, native):
    root = str(tmp_path_factory.mktemp("idata")) + "/"
    native.synth_cohort(root, patients=2, min_slices=3, max_slices=3, threads=2)
    return root


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _cli(out, data, *extra, tool="img_processing_parallel"):
    r = run_bin(tool, "--cpu", "--quiet", *extra, "--data-root", data, "--out", str(out), "--json", str(out) + ".json")
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def cpu_2d(small_cohort, tmp_path_factory):
    return _cli(tmp_path_factory.mktemp("icpu") / "out", small_cohort, "--measure-intensity")


@pytest.fixture(scope="module")
def cpu_3d(small_cohort, tmp_path_factory):
    return _cli(tmp_path_factory.mktemp("icpu3") / "out", small_cohort, "--mode", "3d", "--measure-intensity")


def _numpy_check(js, mask_count_key):
    """The sidecar's own integers are consistent (the masks are not exported: the cross-check against a
    sort of the samples is test_cli_cpu_sidecars_equal_the_golden_pipeline's, through the golden run)."""
    ps = [js[f"raw_p{p}"] for p in ic.PERCENTILES]
    if js[mask_count_key]:
        assert js["raw_min"] <= ps[0] and ps == sorted(ps) and ps[-1] <= js["raw_max"]
        assert js["raw_sum_sq"] * js[mask_count_key] >= js["raw_sum"] ** 2
    else:
        assert ps == [0] * 5 and js["raw_sum_sq"] == 0 and js["std"] is None


def test_cli_cpu_sidecars_equal_the_golden_pipeline_2d(native, small_cohort, cpu_2d, tmp_path):
    import nm03_capstone_project_amd as nm
    from nm03_capstone_project_amd.utils import read_measurements
    base = native.cohort_dir(small_cohort)
    files = [(pid, f) for pid in native.find_patient_dirs(base) for f in native.list_patient_series(base, pid)[1]]
    assert len(files) == 6
    pipe = nm.SlicePipeline(nm.PipelineConfig(measure_intensity=True))
    plain = nm.SlicePipeline(nm.PipelineConfig(measure=True))
    rows = read_measurements(str(cpu_2d))
    some = 0
    for pid, f in files:
        raw, meta = native.read_slice(f, 0)
        stem = os.path.splitext(os.path.basename(f))[0]
        text = (cpu_2d / pid / f"{stem}_measure.json").read_bytes().decode()
        g = pipe.golden(raw, meta)
        assert text == g["measure_json"]
        g0 = plain.golden(raw, meta)
        assert "intensity" not in g0 and text.startswith(g0["measure_json"][:-2] + ',"raw_sum_sq":')
        js = json.loads(text)
        # the integers against a sort of the samples under the golden run's dilated mask, in NumPy
        ref = reference.measure_intensity(g["dilated"], raw, meta["type"], int(meta["stored_bits"]))
        assert g["intensity"] == ref and {k: js[k] for k in ic.INT_KEYS} == {k: ref[k] for k in ic.INT_KEYS}
        assert ref["count"] == js["area_px"]
        _numpy_check(js, "area_px")
        some += ref["count"] > 0
        row = [r for r in rows if r["patient"] == pid and r["file"] == os.path.basename(f)][0]
        assert {k: row[k] for k in NEW_COLUMNS} == {k: js[k] for k in NEW_COLUMNS}
    assert some, "empty masks prove nothing"
    header = (cpu_2d / "measurements.csv").read_text().splitlines()[0].split(",")
    assert header[-13:] == NEW_COLUMNS and len(header) == 3 + 24 + 13
    for r in rows:
        if r["file"] == "TOTAL":
            assert all(r[k] is None for k in NEW_COLUMNS) and r["area_px"] is not None
    j = json.load(open(str(cpu_2d) + ".json"))
    assert j["measure"]["intensity"] is True and j["measure"]["slices"] == 6
    # without the flag: the parent's header, the parent's sidecars (the prefix), the parent's totals object
    out = _cli(tmp_path / "plain", small_cohort, "--measure")
    t, with_flag = tree(out), tree(cpu_2d)
    assert set(t) == set(with_flag)
    for name, data in t.items():
        if name.endswith("_measure.json"):
            assert "raw_p50" not in json.loads(data) and with_flag[name].startswith(data[:-2] + b",")
        elif name == "measurements.csv":
            lines, flines = data.decode().splitlines(), with_flag[name].decode().splitlines()
            assert lines[0].split(",") == header[:-13] and all(len(ln.split(",")) == 27 for ln in lines)
            assert [",".join(ln.split(",")[:-13]) for ln in flines] == lines
        else:
            assert data == with_flag[name], name
    assert set(json.load(open(str(out) + ".json"))["measure"]) == {"slices", "area_px_total", "area_mm2_total"}


def test_cli_cpu_with_diameters_ranks_sequential_and_resume(small_cohort, cpu_2d, tmp_path):
    both = tree(_cli(tmp_path / "both", small_cohort, "--measure-intensity", "--measure-diameters"))
    dia = tree(_cli(tmp_path / "dia", small_cohort, "--measure-diameters"))
    for name, data in dia.items():
        if name.endswith("_measure.json"):
            assert both[name].startswith(data[:-2] + b',"raw_sum_sq":')
            assert list(json.loads(both[name]))[-13:] == NEW_COLUMNS
    head = both["measurements.csv"].decode().splitlines()[0].split(",")
    assert head[-13:] == NEW_COLUMNS and head[:-13] == dia["measurements.csv"].decode().splitlines()[0].split(",")
    # any rank count, the sequential CLI
    assert tree(_cli(tmp_path / "two", small_cohort, "--measure-intensity", "--gpus", "2")) == tree(cpu_2d)
    assert tree(_cli(tmp_path / "seq", small_cohort, "--measure-intensity", tool="img_processing_sequential")) == tree(cpu_2d)
    # --resume leaves a finished tree as it is
    out = _cli(tmp_path / "res", small_cohort, "--measure-intensity")
    before = tree(out)
    _cli(out, small_cohort, "--measure-intensity", "--resume")
    assert tree(out) == before == tree(cpu_2d)
    # ... and counts an older sidecar as done: the new columns stay empty
    old = _cli(tmp_path / "old", small_cohort, "--measure")
    b = tree(old)
    _cli(old, small_cohort, "--measure-intensity", "--resume")
    a = tree(old)
    assert {k: v for k, v in a.items() if k != "measurements.csv"} == {k: v for k, v in b.items() if k != "measurements.csv"}
    lines = a["measurements.csv"].decode().splitlines()
    assert lines[0].split(",")[-13:] == NEW_COLUMNS
    assert all(ln.split(",")[-13:] == [""] * 13 for ln in lines[1:]) and all(ln.split(",")[2] in ("ok", "") for ln in lines[1:])
    assert [",".join(ln.split(",")[:-13]) for ln in lines] == b["measurements.csv"].decode().splitlines()


def test_cli_cpu_3d_sidecars_and_table(native, small_cohort, cpu_3d, tmp_path):
    from nm03_capstone_project_amd.utils import read_volume_measurements
    t = tree(cpu_3d)
    plain = tree(_cli(tmp_path / "plain", small_cohort, "--mode", "3d", "--measure-volume"))
    les = tree(_cli(tmp_path / "les", small_cohort, "--mode", "3d", "--measure-intensity", "--measure-volume-lesions", "2"))
    assert set(t) == set(plain) and set(les) - set(t) == {"lesions.csv"}
    sides = [k for k in t if k.endswith("volume_measure.json")]
    assert len(sides) == 2
    rows = read_volume_measurements(str(cpu_3d))
    for k in sides:
        assert t[k].startswith(plain[k][:-2] + b',"raw_sum_sq":')
        js = json.loads(t[k])
        assert list(js)[-13:] == NEW_COLUMNS and list(js)[:-13] == list(json.loads(plain[k]))
        _numpy_check(js, "volume_vox")
        jl = json.loads(les[k])
        assert list(jl)[-2:] == ["lesions_max", "lesions"] and list(jl)[:-2] == list(js)
        assert {c: jl[c] for c in NEW_COLUMNS} == {c: js[c] for c in NEW_COLUMNS}
        row = [r for r in rows if r["patient"] == os.path.dirname(k)][0]
        assert {c: row[c] for c in NEW_COLUMNS} == {c: js[c] for c in NEW_COLUMNS}
    head = t["volumes.csv"].decode().splitlines()
    assert head[0].split(",")[-13:] == NEW_COLUMNS
    assert [",".join(ln.split(",")[:-13]) for ln in head] == plain["volumes.csv"].decode().splitlines()
    assert all(t[k] == plain[k] for k in t if k not in sides and k != "volumes.csv")
    assert les["volumes.csv"] == t["volumes.csv"]
    assert json.load(open(str(cpu_3d) + ".json"))["measure_volume"]["intensity"] is True
    assert "intensity" not in json.load(open(str(tmp_path / "plain") + ".json"))["measure_volume"]
    # --resume leaves the tree as it is
    _cli(cpu_3d, small_cohort, "--mode", "3d", "--measure-intensity", "--resume")
    assert tree(cpu_3d) == t


@pytest.mark.parametrize("tool", ["img_processing_parallel", "img_processing_sequential"])
def test_flag_is_refused_with_split_volume(tool, cohort_root, tmp_path):
    r = run_bin(tool, "--mode", "3d", "--split-volume", "--measure-intensity", "--data-root", cohort_root, "--out",
                str(tmp_path / "o"))
    assert r.returncode == 2 and "--measure-intensity is not available with --split-volume" in r.stderr
    assert "unknown option" not in r.stderr and not (tmp_path / "o").exists()


def test_engine_rejects_the_flag_on_the_host_path(native):
    import nm03_capstone_project_amd as nm
    with pytest.raises(ValueError, match="measure"):
        native.Engine(nm.PipelineConfig(batch_size=1, streams=1, threads=1, measure_intensity=True, host_only=True).engine_config())


def test_test_pipeline_cpu_extends_measure_json(native, cohort_root, tmp_path):
    import nm03_capstone_project_amd as nm
    ms, it = tmp_path / "ms", tmp_path / "it"
    assert run_bin("test_pipeline", "--cpu", "--measure", "--data-root", cohort_root, "--out", str(ms)).returncode == 0
    r = run_bin("test_pipeline", "--cpu", "--measure-intensity", "--data-root", cohort_root, "--out", str(it))
    assert r.returncode == 0, r.stderr
    a, b = tree(ms), tree(it)
    assert set(a) == set(b) and all(a[k] == b[k] for k in a if k != "measure.json")
    assert b["measure.json"].startswith(a["measure.json"][:-2] + b',"raw_sum_sq":')
    raw, meta = native.read_slice(native.test_slice_path(cohort_root), 0)
    g = nm.SlicePipeline(nm.PipelineConfig(measure_intensity=True)).golden(raw, meta)
    assert b["measure.json"].decode() == g["measure_json"] and g["intensity"]["count"] > 0


def test_flag_in_help():
    r = run_bin("img_processing_parallel", "--help")
    assert r.returncode == 0 and "--measure-intensity" in r.stdout


def test_volume_pipeline_rejects_intensity_without_measure():
    import nm03_capstone_project_amd as nm
    with pytest.raises(ValueError):
        nm.VolumePipeline(measure_intensity=True)
