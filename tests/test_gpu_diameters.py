"""--measure-diameters on the MI355X: the K9 kernel (k9_diameters.hip, on K7's labelling) against the golden
model, field for field; the engine's sidecars; the CLIs. Every compared value is an integer or a string
from the one shared to_json: no tolerance anywhere."""
import json
import os

import numpy as np
import pytest

import diameter_masks as dm
from conftest import run_bin

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def m():
    import nm03_capstone_project_amd as mod
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return mod


def _gpu(m, masks, conn):
    return [dict(r) for r in m.ops.measure_diameters([torch.from_numpy(np.array(k)).cuda() for k in masks], conn)]


def _golden(m, mask, conn):
    return dict(m.native().golden_measure_diameters(mask.astype(np.uint8), conn))


# (100,100): the engine's minimum. (77,131): partial last word. (256,256): the cohort's shape, full last
# word. (520,600): more words than threads. (1100,70): more rows than threads — the row-extreme arrays
# and the pair loop stride past 1024.
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(100, 100), (77, 131), (256, 256), (520, 600), (1100, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_measure_diameters_equals_golden_on_every_named_mask(m, shape, conn):
    """Every named mask of one shape in ONE launch (one workgroup per mask), each compared with the golden."""
    h, w = shape
    masks = [dm.build(name, h, w) for name in dm.NAMES]
    got = _gpu(m, masks, conn)
    assert len(got) == len(dm.NAMES)
    for name, mask, g in zip(dm.NAMES, masks, got):
        assert g == _golden(m, mask, conn), name


def test_mixed_sizes_in_one_launch(m):
    """Masks of four sizes in one launch equal their per-mask launches: descriptor offsets, scratch strides."""
    shapes = [(100, 100), (256, 256), (77, 131), (520, 600)]
    names = ["frame_and_disc", "noise_0.593", "word_span", "rings3"]
    masks = [dm.build(n, h, w) for n, (h, w) in zip(names, shapes)]
    batch = _gpu(m, masks, 8)
    for k in range(4):
        assert batch[k] == _gpu(m, [masks[k]], 8)[0], shapes[k]
        assert batch[k] == _golden(m, masks[k], 8), shapes[k]
    assert len({b["major_px2"] for b in batch}) == 4


def test_takes_stacked_tensors(m):
    masks = np.stack([dm.build("ring", 100, 100), dm.build("two_equal", 100, 100), dm.build("empty", 100, 100)])
    got = [dict(r) for r in m.ops.measure_diameters(torch.from_numpy(masks).cuda(), 4)]
    assert got == [_golden(m, masks[i], 4) for i in range(3)]
    assert got[1]["lesion_first"] == [60, 5] and got[2]["major"] == [-1] * 4
    one = m.ops.measure_diameters(torch.from_numpy(masks[0]).cuda())
    assert len(one) == 1 and dict(one[0]) == _golden(m, masks[0], 8)


@pytest.mark.parametrize("conn", [8, 4])
def test_run_array_matches_golden(m, conn):
    n = m.native()
    raw = n.phantom_slice(256, 256, 3, 12, 25, 7)
    meta = {"type": "u16", "stored_bits": 16, "slope": 2.0, "intercept": -100.0, "spacing_x": 0.9, "spacing_y": 1.1}
    cfg = m.PipelineConfig(batch_size=1, streams=1, threads=2, measure_diameters=True, measure_connectivity=conn)
    pipe = m.SlicePipeline(cfg)
    ref = pipe.golden(raw, meta)
    gpu = pipe.run_array(raw, meta)
    assert ref["diameters"]["lesion_px"] > 1 and ref["diameters"]["major_px2"] > 0, "an empty lesion proves nothing"
    assert dict(gpu["diameters"]) == dict(ref["diameters"])
    assert gpu["measure"] == ref["measure"]
    assert gpu["measure_json"] == ref["measure_json"]
    assert '"bidimensional_mm2":' in gpu["measure_json"]
    plain = m.SlicePipeline(cfg.replace(measure_diameters=False)).run_array(raw, meta)
    assert "diameters" not in plain and "measure" not in plain and plain["jpegs"] == gpu["jpegs"]


def _items(native, root, out):
    base = native.cohort_dir(root)
    items = []
    for pid in native.find_patient_dirs(base):
        _, files = native.list_patient_series(base, pid)
        od = os.path.join(out, pid)
        os.makedirs(od, exist_ok=True)
        items += [(f, od) for f in files]
    return items


def _tree(d):
    res = {}
    for dp, _, fs in os.walk(d):
        for f in fs:
            p = os.path.join(dp, f)
            res[os.path.relpath(p, d)] = open(p, "rb").read()
    return res


def test_engine_cohort(m, tmp_path):
    """6 patients × 5 slices: every sidecar equals the golden's string; the other files are those of a
    --measure run, whose sidecars are the prefixes of these."""
    n = m.native()
    root = str(tmp_path / "data") + "/"
    n.synth_cohort(root, patients=6, min_slices=5, max_slices=5, threads=4)
    cfg = m.PipelineConfig(batch_size=8, streams=2, threads=8, measure_diameters=True)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    items = _items(n, root, on)
    assert len(items) == 30
    st, _ = n.Engine(cfg.engine_config()).run(items)
    assert all(c == 0 for c, _ in st), st
    st, _ = n.Engine(cfg.replace(measure_diameters=False, measure=True).engine_config()).run(_items(n, root, off))
    assert all(c == 0 for c, _ in st), st
    t_on, t_off = _tree(on), _tree(off)
    assert len(t_on) == 90 and set(t_on) == set(t_off)
    lesions = 0
    gold = m.SlicePipeline(cfg)
    for f, od in items:
        raw, meta = n.read_slice(f)
        g = gold.golden(raw, meta)
        key = os.path.relpath(os.path.join(od, os.path.splitext(os.path.basename(f))[0]), on)
        assert t_on[key + "_measure.json"].decode() == g["measure_json"], key
        assert t_on[key + "_measure.json"].decode().startswith(t_off[key + "_measure.json"].decode()[:-2] + ',"lesion_px":')
        lesions += g["diameters"]["major_px2"] > 0
    assert lesions > 0
    assert {k: v for k, v in t_on.items() if not k.endswith("_measure.json")} == \
        {k: v for k, v in t_off.items() if not k.endswith("_measure.json")}


def test_cli_trees(m, cohort_root, tmp_path):
    """img_processing_parallel --measure-diameters equals --cpu tree for tree, measurements.csv included;
    two ranks sharing device 0 equal one."""
    env = {"NM03_DEVICE_OVERRIDE": "0", "NM03_COMM_TIMEOUT_S": "60"}
    trees = {}
    for name, extra in (("gpu1", ["--gpus", "1", "--threads", "4"]), ("gpu2", ["--gpus", "2", "--threads", "4"]),
                        ("cpu", ["--cpu"])):
        out = tmp_path / name
        r = run_bin("img_processing_parallel", "--measure-diameters", *extra, "--quiet", "--data-root", cohort_root, "--out",
                    str(out), env=env, timeout=240)
        assert r.returncode == 0, (name, r.stderr)
        trees[name] = _tree(str(out))
    assert b"bidimensional_mm2" in trees["gpu1"]["measurements.csv"]
    assert trees["gpu1"] == trees["cpu"]
    assert trees["gpu2"] == trees["gpu1"]


def test_test_pipeline_gpu(m, cohort_root, tmp_path):
    cpu, gpu = tmp_path / "cpu", tmp_path / "gpu"
    for out, extra in ((cpu, ["--cpu"]), (gpu, [])):
        r = run_bin("test_pipeline", *extra, "--measure-diameters", "--data-root", cohort_root, "--out", str(out))
        assert r.returncode == 0, r.stderr
    assert (gpu / "measure.json").read_bytes() == (cpu / "measure.json").read_bytes()
    assert json.loads((gpu / "measure.json").read_text())["major_px2"] > 0
