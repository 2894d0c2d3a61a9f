"""--measure on the MI355X: the K7 kernel (k7_measure.hip) against the golden model, field for field,
on the masks a labelling kernel gets wrong; the engine's sidecars; the cohort CLIs. Every compared
value is an integer or a string from the one shared to_json: no tolerance anywhere."""
import os

import numpy as np
import pytest

import measure_masks as mm
from conftest import run_bin

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def m():
    import nm03_capstone_project_amd as mod
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return mod


def _gpu(m, masks, raws, conn, pixel_type="u16", bits=16):
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # a copy: the cached masks are read-only
    return m.ops.measure_mask([dev(k) for k in masks], [dev(mm.region_of(k)) for k in masks],
                              [dev(r.view(np.int16)) for r in raws], conn, pixel_type, bits)


def _golden(m, mask, raw, conn, pixel_type="u16", bits=16):
    return m.native().golden_measure(mask.astype(np.uint8), mm.region_of(mask).astype(np.uint8), raw, pixel_type, bits, conn)


# (100,100): the engine's minimum. (77,131): three words per row, partial last word. (256,256): the
# cohort's shape, full last word. (520,600): above kSrgMaxDim, ten words per row, more words than threads.
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(100, 100), (77, 131), (256, 256), (520, 600)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_measure_mask_equals_golden_on_every_named_mask(m, shape, conn):
    """Every named mask of one shape in ONE launch (one workgroup per mask), each compared with the golden."""
    h, w = shape
    masks = [mm.build(name, h, w) for name in mm.NAMES]
    raw = mm.raw_of(h, w)
    got = _gpu(m, masks, [raw] * len(masks), conn)
    assert len(got) == len(mm.NAMES)
    for name, mask, g in zip(mm.NAMES, masks, got):
        assert g == _golden(m, mask, raw, conn), name


@pytest.mark.parametrize("conn", [4, 8])
def test_measure_mask_512_adversarial(m, conn):
    """512²: the checkerboard (131,072 components at 4-connectivity), the serpentines (one component, the
    longest merge chains) and percolation-threshold noise (the raggedest components)."""
    names = ["checkerboard", "serpentine", "serpentine_v", "spiral", "noise_0.593"]
    masks = [mm.build(name, 512, 512) for name in names]
    raw = mm.raw_of(512, 512)
    got = _gpu(m, masks, [raw] * len(masks), conn)
    for name, mask, g in zip(names, masks, got):
        assert g == _golden(m, mask, raw, conn), name
    assert got[0]["components"] == (131072 if conn == 4 else 1)
    assert got[1]["components"] == 1 and got[2]["components"] == 1


def test_measure_mask_mixed_sizes_in_one_launch(m):
    """Slices of four sizes in one launch_measure equal their per-slice results: descriptor offsets, scratch strides."""
    shapes = [(100, 100), (256, 256), (77, 131), (512, 512)]
    names = ["rings3", "noise_0.593", "word_edges", "comb"]
    masks = [mm.build(n, h, w) for n, (h, w) in zip(names, shapes)]
    raws = [mm.raw_of(h, w, seed=5) for h, w in shapes]
    batch = _gpu(m, masks, raws, 8)
    for k in range(4):
        assert batch[k] == _gpu(m, [masks[k]], [raws[k]], 8)[0], shapes[k]
        assert batch[k] == _golden(m, masks[k], raws[k], 8), shapes[k]
    assert len({b["area_px"] for b in batch}) == 4


@pytest.mark.parametrize("pixel_type,bits", [("i16", 16), ("u16", 12)])
def test_measure_mask_intensities(m, pixel_type, bits):
    """Signed 16-bit and unsigned 12-bit stored samples under the ring, against NumPy."""
    mask = mm.build("ring", 100, 100)
    raw = mm.raw_of(100, 100, seed=9)
    got = _gpu(m, [mask], [raw], 8, pixel_type, bits)[0]
    v = raw.view(np.int16).astype(np.int64) if pixel_type == "i16" else (raw.astype(np.int64) & 0xFFF)
    assert (got["raw_sum"], got["raw_min"], got["raw_max"]) == (int(v[mask].sum()), int(v[mask].min()), int(v[mask].max()))
    assert got == _golden(m, mask, raw, 8, pixel_type, bits)
    assert got["holes"] == 1 and got["components"] == 1


def test_measure_mask_takes_stacked_tensors(m):
    masks = np.stack([mm.build("ring", 100, 100), mm.build("comb", 100, 100)])
    raw = np.stack([mm.raw_of(100, 100)] * 2)
    reg = np.stack([mm.region_of(k) for k in masks])
    got = m.ops.measure_mask(torch.from_numpy(masks).cuda(), torch.from_numpy(reg).cuda(),
                             torch.from_numpy(raw.view(np.int16)).cuda(), 4)
    assert got == [_golden(m, masks[i], raw[i], 4) for i in range(2)]
    with pytest.raises(ValueError):
        m.ops.measure_mask(torch.from_numpy(masks).cuda(), torch.from_numpy(reg[:1]).cuda(),
                           torch.from_numpy(raw.view(np.int16)).cuda())


@pytest.mark.parametrize("conn", [8, 4])
def test_run_array_measure_matches_golden(m, conn):
    n = m.native()
    raw = n.phantom_slice(256, 256, 3, 12, 25, 7)
    meta = {"type": "u16", "stored_bits": 16, "slope": 2.0, "intercept": -100.0, "spacing_x": 0.9, "spacing_y": 1.1}
    cfg = m.PipelineConfig(batch_size=1, streams=1, threads=2, measure=True, measure_connectivity=conn)
    pipe = m.SlicePipeline(cfg)
    ref = pipe.golden(raw, meta)
    gpu = pipe.run_array(raw, meta)
    assert ref["measure"]["area_px"] > 0 and ref["measure"]["region_px"] > 0, "an empty mask proves nothing"
    assert gpu["measure"] == ref["measure"]
    assert gpu["measure_json"] == ref["measure_json"]
    plain = m.SlicePipeline(cfg.replace(measure=False)).run_array(raw, meta)
    assert "measure" not in plain and "measure_json" not in plain and plain["jpegs"] == gpu["jpegs"]


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


def test_engine_cohort_measure(m, tmp_path):
    """6 patients × 5 slices: every sidecar equals the golden's string, the JPEGs are those of a run without
    the flag, which writes no sidecar; --resume counts a slice done only when its sidecar exists too."""
    n = m.native()
    root = str(tmp_path / "data") + "/"
    n.synth_cohort(root, patients=6, min_slices=5, max_slices=5, threads=4)
    cfg = m.PipelineConfig(batch_size=8, streams=2, threads=8, measure=True)
    on, off = str(tmp_path / "on"), str(tmp_path / "off")
    items = _items(n, root, on)
    assert len(items) == 30
    st, _ = n.Engine(cfg.engine_config()).run(items)
    assert all(c == 0 for c, _ in st), st
    st, _ = n.Engine(cfg.replace(measure=False).engine_config()).run(_items(n, root, off))
    assert all(c == 0 for c, _ in st), st
    t_on, t_off = _tree(on), _tree(off)
    assert len(t_off) == 60 and len(t_on) == 90
    assert not any(k.endswith("_measure.json") for k in t_off)
    assert {k: v for k, v in t_on.items() if not k.endswith("_measure.json")} == t_off
    areas = 0
    for f, od in items:
        raw, meta = n.read_slice(f)
        g = m.SlicePipeline(cfg).golden(raw, meta)
        key = os.path.relpath(os.path.join(od, os.path.splitext(os.path.basename(f))[0]), on)
        assert t_on[key + "_measure.json"].decode() == g["measure_json"], key
        areas += g["measure"]["area_px"]
    assert areas > 0
    victim = os.path.join(items[3][1], os.path.splitext(os.path.basename(items[3][0]))[0] + "_measure.json")
    os.remove(victim)
    st, _ = n.Engine(cfg.replace(resume=True).engine_config()).run(items)
    assert [msg.startswith("resumed") for _, msg in st].count(False) == 1 and not st[3][1].startswith("resumed")
    assert _tree(on) == t_on


def test_cli_measure_trees(m, cohort_root, tmp_path):
    """img_processing_parallel --measure equals --cpu --measure tree for tree, measurements.csv included;
    two ranks sharing device 0 equal one; without the flag no sidecar and no table."""
    env = {"NM03_DEVICE_OVERRIDE": "0", "NM03_COMM_TIMEOUT_S": "60"}
    trees = {}
    for name, extra in (("gpu1", ["--measure", "--gpus", "1", "--threads", "4"]),
                        ("gpu2", ["--measure", "--gpus", "2", "--threads", "4"]),
                        ("cpu", ["--measure", "--cpu"]),
                        ("off", ["--gpus", "1", "--threads", "4"])):
        out = tmp_path / name
        r = run_bin("img_processing_parallel", *extra, "--quiet", "--data-root", cohort_root, "--out", str(out), env=env,
                    timeout=240)
        assert r.returncode == 0, (name, r.stderr)
        trees[name] = _tree(str(out))
    assert "measurements.csv" in trees["gpu1"]
    assert trees["gpu1"] == trees["cpu"]
    assert trees["gpu2"] == trees["gpu1"]
    assert {k: v for k, v in trees["gpu1"].items() if not k.endswith("_measure.json") and k != "measurements.csv"} == trees["off"]
    assert 3 * len(trees["off"]) // 2 + 1 == len(trees["gpu1"])


def test_test_pipeline_gpu_measure(m, cohort_root, tmp_path):
    cpu, gpu = tmp_path / "cpu", tmp_path / "gpu"
    for out, extra in ((cpu, ["--cpu"]), (gpu, [])):
        r = run_bin("test_pipeline", *extra, "--measure", "--data-root", cohort_root, "--out", str(out))
        assert r.returncode == 0, r.stderr
    assert (gpu / "measure.json").read_bytes() == (cpu / "measure.json").read_bytes()
    assert b'"area_px":' in (gpu / "measure.json").read_bytes()
