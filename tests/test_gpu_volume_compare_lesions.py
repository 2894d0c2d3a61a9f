"""K18 (--compare-lesions) on the GPU against the golden model, everything compared with ==:
  test_op_equals_golden                 ops.compare_volume_lesions on every case of volume_compare_lesion_cases at
                                        N = 1, 2, 64, at c = 6 and 26, both orders of the masks; the size case at
                                        max_blocks 1, 5 and the default
  test_op_words_with_bits_past_the_width   the op's flat-word form on words whose bits past the width are set
  test_op_refusals                      every ValueError of the op, with one good call after them
  test_pipeline_compare_lesions         VolumePipeline(compare_to=..., compare_lesions=N) with the cube and with
                                        dilate_mm: the record, the text, and a run against its own mask
  test_cli_tree_equals_cpu_tree         the GPU CLI's tree == the --cpu tree
  test_flag_leaves_flagless_runs_unchanged   a run with the flag, then one without, on one runner
  test_run_slab_refuses_and_run_checks_first"""
import json
import os

import numpy as np
import pytest

import volume_compare_lesion_cases as lc
import volume_export_cases as xc
from conftest import run_bin

pytestmark = pytest.mark.gpu

CASES = lc.cases()


def tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def golden(native):
    """The golden record of every case, N and connectivity, computed once."""
    return {(c["name"], n, conn): lc.plain(native.golden_compare_volume_lesions(c["a"], c["b"], n, conn))
            for c in CASES for n in lc.NS for conn in (6, 26)}


@pytest.mark.parametrize("c", CASES, ids=lc.ids(CASES))
def test_op_equals_golden(native, golden, c):
    import torch
    import nm03_capstone_project_amd as nm
    a = torch.from_numpy(np.array(c["a"])).cuda().bool()
    b = torch.from_numpy(np.array(c["b"])).cuda().bool()
    for n in lc.NS:
        for conn in (6, 26):
            g = golden[(c["name"], n, conn)]
            for mb in c["max_blocks"]:  # the cap changes the trips, never the record
                got = nm.ops.compare_volume_lesions(a, b, n, conn, max_blocks=mb)
                assert tuple(got) == lc.DICT_KEYS and got["table"].dtype == torch.int64 and tuple(got["table"].shape) == (n + 1, n + 1)
                assert lc.plain(got) == g, (n, conn, mb)
                assert lc.plain(nm.ops.compare_volume_lesions(b, a, n, conn, max_blocks=mb)) == lc.swapped(g), (n, conn, mb)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["width_63", "width_65", "width_130", "lattice", "worked_row", "size"])
def test_op_words_with_bits_past_the_width(native, golden, name):
    import torch
    import nm03_capstone_project_amd as nm
    c = lc.case(name)
    d, h, w = c["a"].shape
    assert w % 64 != 0
    junk = torch.tensor(-1 << (w % 64), dtype=torch.int64, device="cuda")  # every bit past the width in a row's last word
    words = []
    for m in (c["a"], c["b"]):
        wd = nm.ops.pack_bits(torch.from_numpy(np.array(m)).cuda().bool()).contiguous().clone()
        wd[:, :, -1] |= junk
        words.append(wd)
    for n, conn in ((2, 6), (64, 26)):
        got = nm.ops.compare_volume_lesions_words(words[0], words[1], w, n, conn)
        assert lc.plain(got) == golden[(name, n, conn)]
    torch.cuda.synchronize()


def test_op_refusals(native):
    import torch
    import nm03_capstone_project_amd as nm
    m = torch.ones((3, 4, 5), dtype=torch.bool, device="cuda")
    for bad in ((m.cpu(), m, 2), (m, m.cpu(), 2), (m[0], m[0], 2), (m, m[:, :, :4], 2), (m, m, 0), (m, m, 65), (m, m, 2, 18)):
        with pytest.raises(ValueError):
            nm.ops.compare_volume_lesions(*bad)
    with pytest.raises(ValueError):
        nm.ops.compare_volume_lesions(m, m, 2, max_blocks=0)
    wd = nm.ops.pack_bits(m)
    with pytest.raises(ValueError):
        nm.ops.compare_volume_lesions_words(wd, wd, 65, 2)  # one word per row cannot hold 65 voxels
    with pytest.raises(ValueError):
        nm.ops.compare_volume_lesions_words(wd.int(), wd.int(), 5, 2)
    with pytest.raises(ValueError, match="connectivity must be 6 or 26"):
        native.k_volume_compare_lesions(wd.data_ptr(), wd.data_ptr(), 5, 4, 3, 2, 18)
    with pytest.raises(ValueError, match="null buffer"):
        native.k_volume_compare_lesions(0, wd.data_ptr(), 5, 4, 3, 2, 26)
    with pytest.raises(ValueError, match="must stay below 2\\^32"):
        native.k_volume_compare_lesions(wd.data_ptr(), wd.data_ptr(), 65535, 65535, 2, 2, 26)
    got = nm.ops.compare_volume_lesions(m, m, 2)  # the runtime goes on afterwards
    assert (got["lesions_a"], got["hit_a"], got["multi_a"], got["lesions_b"], got["hit_b"], got["multi_b"]) == (1, 1, 0, 1, 1, 0)
    assert got["table"].tolist() == [[60, 0, 0], [0, 0, 0], [0, 0, 0]] and got["a_lesions"][0]["best"] == 0


# ---- the runner ---------------------------------------------------------------------------------------
VOL_SHAPE = (5, 104, 136)  # d, h, w: the phantom of test_gpu_volume_compare.py
VOL_SPACING = (0.5, 0.75, 5.0)
VOL_UM = [500, 750, 5000]
N_RUN = 4


@pytest.fixture(scope="module")
def volume(native):
    d, h, w = VOL_SHAPE
    s0 = xc.slice0(d)
    planes = np.stack([native.phantom_slice(h, w, 3, s0 + k, xc.NSLICES, xc.SEED) for k in range(d)]).astype(np.uint16)
    planes.setflags(write=False)
    return planes


@pytest.fixture(scope="module")
def cube_mask(native, volume):
    import nm03_capstone_project_amd as nm
    res = nm.VolumePipeline(nm.PipelineConfig()).run(volume)
    assert res["dilated"].sum() > res["region"].sum() > 0
    return res["dilated"]


@pytest.mark.parametrize("kw", [dict(dilate_mm=2.5), dict(), dict(dilate_mm=0, measure=True, measure_lesions=2, measure_connectivity=6)],
                         ids=["dilate_mm", "cube", "with_measures_c6"])
def test_pipeline_compare_lesions(native, volume, cube_mask, kw):
    import nm03_capstone_project_amd as nm
    pipe = nm.VolumePipeline(nm.PipelineConfig(), compare_to=cube_mask, compare_reference="cube", compare_lesions=N_RUN, **kw)
    res = pipe.run(volume, spacing=VOL_SPACING)
    plain = nm.VolumePipeline(nm.PipelineConfig(), compare_to=cube_mask, compare_reference="cube", **kw).run(volume, spacing=VOL_SPACING)
    assert set(res) == set(plain) | {"compare_lesions", "compare_lesions_s"}
    assert np.array_equal(res["dilated"], plain["dilated"]) and res["compare"] == plain["compare"]
    conn = kw.get("measure_connectivity", 26)
    g = native.golden_compare_volume_lesions(res["dilated"], cube_mask, N_RUN, conn)
    assert lc.plain(res["compare_lesions"]) == lc.plain(g) and g["lesions_b"] >= 1 and g["hit_b"] >= 1
    d, h, w = VOL_SHAPE
    assert res["compare_json"] == native.volume_compare_to_json(res["compare"], w, h, d, VOL_UM, "cube", g)
    assert res["compare_json"][:res["compare_json"].index(',"lesions_connectivity"')] + "}\n" == plain["compare_json"]
    js = json.loads(res["compare_json"])
    assert js["lesions_connectivity"] == conn and js["lesions_max"] == N_RUN
    if not kw:  # the cube against the cube: every lesion hit, none multi, f1 == 1
        assert g["hit_a"] == g["lesions_a"] == g["hit_b"] == g["lesions_b"] and g["multi_a"] == g["multi_b"] == 0
        assert js["lesion_f1"] == 1 and js["lesion_sensitivity"] == 1 and js["lesion_precision"] == 1
        assert all(r["best"] == i and r["best_overlap_vox"] == r["voxels"] for i, r in enumerate(g["a_lesions"]))
    if kw.get("measure"):
        for k in ("measure", "measure_json", "lesions"):
            assert res[k] == plain[k], k
        assert [(r["voxels"], r["first"]) for r in g["a_lesions"][:2]] == [(l["voxels"], list(l["first"])) for l in res["lesions"]]


def test_flag_leaves_flagless_runs_unchanged(native, volume, cube_mask):
    import nm03_capstone_project_amd as nm
    kw = dict(measure=True, measure_lesions=2, measure_intensity=True)
    fresh = nm.VolumePipeline(nm.PipelineConfig(), compare_to=cube_mask, **kw).run(volume, spacing=VOL_SPACING)
    pipe = nm.VolumePipeline(nm.PipelineConfig(), compare_to=cube_mask, compare_lesions=N_RUN, **kw)
    flagged = pipe.run(volume, spacing=VOL_SPACING)
    assert set(flagged) == set(fresh) | {"compare_lesions", "compare_lesions_s"}
    pipe.compare_lesions = 0
    after = pipe.run(volume, spacing=VOL_SPACING)
    assert set(after) == set(fresh)
    for k in fresh:
        if k.endswith("_s"):
            continue  # timings
        if isinstance(fresh[k], np.ndarray):
            assert np.array_equal(after[k], fresh[k]), k
        else:
            assert after[k] == fresh[k], k  # compare_json among them: byte-identical to a fresh flagless run


def test_run_slab_refuses_and_run_checks_first(native):
    vol = np.zeros((4, 16, 64), np.uint16)
    ref = np.zeros((4, 16, 64), np.uint8)
    runner = native.VolumeRunner(0)
    with pytest.raises(ValueError, match="lesion-wise comparison of a volume split into slabs"):
        runner.run_slab(native.self_comm(), vol, 0, 4, native.PipelineParams(), 6, 3, [], compare_lesions=2)
    with pytest.raises(ValueError, match="compare_lesions needs a reference"):
        runner.run(vol, native.PipelineParams(), 6, 3, [], compare_lesions=2)
    for n in (-1, 65):
        with pytest.raises(ValueError, match="compare_lesions must be 1..64"):
            runner.run(vol, native.PipelineParams(), 6, 3, [], compare_to=ref, compare_lesions=n)
    with pytest.raises(ValueError, match="connectivity must be 6 or 26"):
        runner.run(vol, native.PipelineParams(), 6, 3, [], compare_to=ref, compare_lesions=2, measure_connectivity=18)
    res = runner.run(vol, native.PipelineParams(), 6, 3, [], compare_to=ref, compare_lesions=2)
    cl = res["compare_lesions"]
    assert cl["lesions_b"] == 0 and cl["hit_a"] == 0 and cl["b_lesions"] == [] and not np.asarray(cl["table"]).any()
    assert cl["lesions_a"] == native.golden_compare_volume_lesions(res["dilated"], ref, 2, 26)["lesions_a"]


# ---- the command-line tool --------------------------------------------------------------------------
def test_cli_tree_equals_cpu_tree(native, tmp_path):
    root = xc.write_cohort(native, tmp_path / "data", xc.formats(native))
    patients = [p["id"] for p in xc.formats(native)]
    ref = tmp_path / "ref"
    r = run_bin("img_processing_parallel", "--mode", "3d", "--quiet", "--gpus", "1", "--volume-mask", "--data-root", root, "--out", str(ref))
    assert r.returncode == 0, r.stderr
    flags = ("--dilate-mm", "2.5", "--compare-to", str(ref), "--compare-lesions", "3", "--measure-volume", "--measure-volume-lesions", "2")
    trees = {}
    for name, extra in (("gpu", ()), ("cpu", ("--cpu",))):
        out = tmp_path / name
        r = run_bin("img_processing_parallel", "--mode", "3d", "--quiet", "--gpus", "1", *extra, *flags, "--data-root", root,
                    "--out", str(out), "--json", str(out) + ".json")
        assert r.returncode == 0, r.stderr
        trees[name] = tree(out)
    assert sorted(trees["gpu"]) == sorted(trees["cpu"]) and "compare_lesions.csv" in trees["gpu"]
    for p in trees["cpu"]:
        assert trees["gpu"][p] == trees["cpu"][p], p
    f1 = []
    for pid in patients:
        js = json.loads(trees["gpu"][os.path.join(pid, "compare.json")])
        assert js["lesions_max"] == 3 and js["lesions_a"] >= 1 and js["hit_b"] >= 1 and len(js["a_lesions"]) == min(3, js["lesions_a"])
        f1.append(js["lesion_f1"])
    run = json.load(open(str(tmp_path / "gpu") + ".json"))
    assert run["compare"]["lesions"] is True and run["compare"]["lesion_f1_mean"] == float("%.9g" % (sum(f1) / len(f1)))
    assert all(p["compare_lesions_s"] > 0 for p in run["patients"])
