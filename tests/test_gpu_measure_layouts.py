"""GPU tests (MI355X) of the measurement kernels K7–K13 on the buffer layouts of their two production hosts,
the 3D VolumeRunner (src/runtime/volume.cpp) and the 2D engine (src/runtime/engine.cpp), which the ops
never produce. Inputs and their CPU conditions: measure_layout_cases.py, test_measure_layout_cases.py. Every
expected value is the golden model's, a NumPy / SciPy reference's or the --cpu run's; every comparison is
of integers, text or bytes.

What each test executes that no other one does:
  test_runner_all_flags_on_the_stride_volumes   K8, K10, K11, K12 with a plane stride of w·h + 1 … w·h + 7
                                                samples (z · stride + y · w + x, K12's partner rows in plane
                                                z + 1), K13 behind them, a partial third mask word, signed
                                                and unsigned volumes alternating on one runner whose buffers
                                                are rebuilt
  test_runner_all_flags_on_the_export_cohorts   the same on 33 signed planes (deep_odd) and on the seven
                                                sample formats (12 stored bits with garbage above, 8 bits,
                                                negative slopes), type and stored bits passed unmapped
  test_cli_3d_all_flags_equal_cpu               the 3D command-line run of both cohorts with every flag
  test_engine_mixed_cohort                      K7, K9, K11, K12 in batches of mixed sizes (raw_off advanced
                                                by the rounded size, 2 to 4 words per row, partial last
                                                words) and formats on two slots, with a failed slice in the
                                                middle of a batch (record c is not slice c of the batch)
  test_engine_resume_redoes_one_slice           a batch of one live slice behind a resumed and a failed one
  test_run_array_on_the_odd_shapes              run_single on the non-256 shapes"""
import os

import numpy as np
import pytest
import torch

import measure_layout_cases as mc
import nm03_capstone_project_amd as nm
import texture_cases as tc
import volume_export_cases as xc
from conftest import run_bin
from nm03_capstone_project_amd.ops import reference as R

pytestmark = pytest.mark.gpu

_TIMEOUT = 240  # as the other 3D CLI tests


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert nm.native().device_count() >= 1


def _tree(d):
    return {os.path.relpath(os.path.join(dp, f), d): open(os.path.join(dp, f), "rb").read()
            for dp, _, fs in os.walk(d) for f in fs}


# ---------------------------------------------------------------------------------------------
# 1. The 3D runner
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipes():
    """One VolumePipeline (one runner, kept across the tests of this module) per measurement connectivity."""
    return {conn: nm.VolumePipeline(measure_connectivity=conn, **mc.VOLUME_KW) for conn in (26, 6)}


@pytest.fixture(scope="module")
def stride_volumes(native):
    return {v["id"]: v for v in mc.stride_volumes(native)}


def _check_volume(native, vp, vol, meta, conn):
    """One run with every flag against the golden model on the run's own masks, and the three records the
    references cover against them."""
    seeds = vp.default_seeds(vol)
    res = vp.run(vol, seeds, meta=meta, **mc.VOLUME_RUN_KW)
    region, dil = vp.golden(res["band"], seeds)
    assert np.array_equal(res["region"], region) and np.array_equal(res["dilated"], dil)
    rec, text, lesions, intensity, texture, diameters = vp.golden_measure(res["dilated"], res["region"], vol, meta=meta,
                                                                          **mc.VOLUME_RUN_KW)
    assert rec["volume_vox"] == int(dil.sum()) > 0 and texture["pairs"] > 0 and len(lesions) >= 1
    assert res["measure"] == rec
    assert res["lesions"] == lesions
    assert res["diameters"] == diameters
    assert res["intensity"] == intensity
    assert tc.same(res["texture"], texture)
    assert res["measure_json"] == text
    ty, bits = meta["type"], meta["stored_bits"]
    assert res["intensity"] == R.measure_intensity(res["dilated"], vol, ty, bits)
    assert tc.same(res["texture"], R.glcm(res["dilated"], vol, mc.STRIDE_LEVELS, ty, bits))
    um = native.volume_spacing_um(float(np.float32(mc.STRIDE_SPACING[0])), float(np.float32(mc.STRIDE_SPACING[1])),
                                  mc.STRIDE_SPACING[2])
    assert res["diameters"] == R.measure_volume_diameters(res["dilated"], mc.STRIDE_LESIONS, um, conn)
    return res


@pytest.mark.parametrize("conn", [26, 6])
@pytest.mark.parametrize("h", mc.STRIDE_HEIGHTS)
def test_runner_all_flags_on_the_stride_volumes(native, pipes, stride_volumes, h, conn):
    """The one runner of `pipes[conn]` meets the seven shapes one after the other, signed and unsigned
    alternating; its buffers are rebuilt whenever the shape changes."""
    v = stride_volumes[f"h{h}"]
    assert mc.padded_stride(h, mc.STRIDE_W) != h * mc.STRIDE_W
    res = _check_volume(native, pipes[conn], v["planes"], v["meta"], conn)
    assert mc.touches_partial_word(res["dilated"])
    assert len(pipes[conn]._runners) == 1


def test_runner_all_flags_on_the_export_cohorts(native, pipes):
    """One deep_odd patient (33 × 101 × 131, signed), then every formats patient in FORMATS order (signed and
    unsigned alternating), on the runner the stride volumes used."""
    vp = pipes[26]
    p = xc.deep_odd(native)[0]
    assert p["planes"].shape == (33, 101, 131) and p["meta"]["type"] == "i16"
    _check_volume(native, vp, p["planes"], p["meta"], 26)
    pts = xc.formats(native)
    assert [q["format"] for q in pts] == list(xc.FORMAT_NAMES)
    for q in pts:
        _check_volume(native, vp, q["planes"], q["meta"], 26)
    assert len(vp._runners) == 1


CLI_FLAGS = ("--measure-volume-lesions", "3", "--measure-volume-diameters", "--measure-intensity", "--measure-texture",
             "--texture-levels", "64")


@pytest.mark.parametrize("name", ["deep_odd", "formats"])
def test_cli_3d_all_flags_equal_cpu(native, tmp_path, name):
    """img_processing_parallel --mode 3d with every measurement flag: the GPU tree is the --cpu tree
    (volumes.csv and lesions.csv included) and its JPEGs are those of the GPU run without a flag."""
    pts = xc.COHORTS[name](native)
    root = xc.write_cohort(native, tmp_path / "data", pts)

    def cli(out, *args):
        r = run_bin("img_processing_parallel", "--mode", "3d", "--quiet", *args, "--data-root", root, "--out",
                    str(tmp_path / out), timeout=_TIMEOUT)
        assert r.returncode == 0, r.stderr
        return _tree(str(tmp_path / out))

    gpu, cpu, plain = cli("gpu", *CLI_FLAGS), cli("cpu", "--cpu", *CLI_FLAGS), cli("plain")
    assert sorted(gpu) == sorted(cpu)
    diffs = sorted(k for k in cpu if gpu[k] != cpu[k])
    assert not diffs, (len(diffs), diffs[:6])
    assert "volumes.csv" in gpu and "lesions.csv" in gpu
    sidecars = [k for k in gpu if k.endswith("volume_measure.json")]
    assert len(sidecars) == len(pts)
    assert all(b'"glcm_levels":64,' in gpu[k] and b'"major_um2":' in gpu[k] and b'"raw_p50":' in gpu[k] for k in sidecars)
    jpegs = {k: v for k, v in gpu.items() if k.endswith(".jpg")}
    assert len(jpegs) == 2 * sum(p["planes"].shape[0] for p in pts)
    assert jpegs == {k: v for k, v in plain.items() if k.endswith(".jpg")}


# ---------------------------------------------------------------------------------------------
# 2. The 2D engine
# ---------------------------------------------------------------------------------------------
def _cfg(**kw):
    return nm.PipelineConfig(**{**mc.ENGINE_CFG, **kw})


def _stem(k):
    return f"1-{k + 1}"


def _run(native, cfg, files, out):
    out.mkdir()
    eng = native.Engine(cfg.engine_config())
    st, times = eng.run([(f, str(out)) for f in files])
    del eng
    return st, times, _tree(str(out))


@pytest.fixture(scope="module")
def engine_files(native, tmp_path_factory):
    return mc.write_engine_set(native, tmp_path_factory.mktemp("mlg") / "in")


@pytest.fixture(scope="module")
def unflagged_tree(native, engine_files, tmp_path_factory):
    """The tree of the same run without the four measurement flags (JPEGs and overlays only)."""
    st, _, tree = _run(native, _cfg(**{k: False for k in mc.MEASURE_FLAGS}), engine_files, tmp_path_factory.mktemp("mlg_off") / "o")
    assert [c for c, _ in st] == [mc.ENGINE_BAD.get(k, (0, ""))[0] for k in range(len(engine_files))]
    assert not any(k.endswith("_measure.json") for k in tree)
    return tree


@pytest.fixture(scope="module")
def golden_sidecars(native, engine_files):
    """levels → {stem: the golden model's sidecar text} of the good slices, computed once per level count."""
    cache = {}

    def get(levels):
        if levels not in cache:
            pipe = nm.SlicePipeline(_cfg(texture_levels=levels))
            cache[levels] = {_stem(k): pipe.golden(*native.read_slice(engine_files[k]))["measure_json"] for k in mc.good_indices()}
        return cache[levels]

    return get


@pytest.mark.parametrize("levels", [64, 7])
def test_engine_mixed_cohort(native, engine_files, unflagged_tree, golden_sidecars, tmp_path, monkeypatch, levels):
    """Twelve files, four batches of three on two slots, with 12-bit packing on and off: statuses 0 except for
    the two bad files, which leave nothing; every sidecar the golden model's text; every JPEG that of the
    unflagged run; both trees byte-identical."""
    cfg = _cfg(texture_levels=levels)
    want = golden_sidecars(levels)
    good = [_stem(k) for k in mc.good_indices()]
    trees = []
    for flag in ("1", "0"):
        monkeypatch.setenv("NM03_PACK12", flag)
        st, times, tree = _run(native, cfg, engine_files, tmp_path / f"o{flag}")
        assert times["batches"] == 4 and times["jpeg_fallbacks"] == 0
        for k, (code, msg) in enumerate(st):
            assert (code, msg) == mc.ENGINE_BAD.get(k, (0, "")), (k, st)
        assert {f.rsplit("_", 1)[0] for f in tree} == set(good), "the bad files have no output at all"
        assert len(tree) == 4 * len(good)
        for stem in good:
            assert tree[stem + "_measure.json"].decode() == want[stem], (stem, flag)
        assert {k: v for k, v in tree.items() if not k.endswith("_measure.json")} == unflagged_tree
        trees.append(tree)
    assert trees[0] == trees[1]
    assert all(f'"glcm_levels":{levels},' in want[s] for s in good)


def test_engine_resume_redoes_one_slice(native, engine_files, golden_sidecars, tmp_path):
    """A sidecar deleted, then resume=True: only that slice is redone (the bad files fail as before) and the
    tree is as it was. The victim follows the too-small file in its batch, whose first slice is resumed, so
    its record is not at its position in the batch."""
    cfg = _cfg()
    st, _, before = _run(native, cfg, engine_files, tmp_path / "o")
    victim = 5
    assert victim - 1 in mc.ENGINE_BAD and victim // mc.ENGINE_BATCH == (victim - 1) // mc.ENGINE_BATCH
    os.remove(tmp_path / "o" / (_stem(victim) + "_measure.json"))
    eng = native.Engine(cfg.replace(resume=True).engine_config())
    st, _ = eng.run([(f, str(tmp_path / "o")) for f in engine_files])
    del eng
    for k, (code, msg) in enumerate(st):
        if k in mc.ENGINE_BAD:
            assert (code, msg) == mc.ENGINE_BAD[k], k
        else:
            assert code == 0 and msg.startswith("resumed") == (k != victim), (k, msg)
    after = _tree(str(tmp_path / "o"))
    assert after == before
    assert after[_stem(victim) + "_measure.json"].decode() == golden_sidecars(64)[_stem(victim)]


@pytest.mark.parametrize("shape,fmt", mc.RUN_ARRAY_CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_run_array_on_the_odd_shapes(native, shape, fmt):
    k = next(i for i, s in enumerate(mc.ENGINE_SLICES) if s[:2] == (shape, fmt) and s[2] is None)
    raw, _, meta = mc.engine_slice(native, k)
    pipe = nm.SlicePipeline(_cfg(streams=1, batch_size=1))
    r, g = pipe.run_array(raw, meta), pipe.golden(raw, meta)
    ty, bits = meta["type"], meta["stored_bits"]
    for key in ("band", "region", "dilated"):
        assert np.array_equal(r[key], g[key].astype(bool)), key
    assert r["dilated"].any() and mc.touches_partial_word(r["dilated"])
    assert r["intensity"] == g["intensity"] == R.measure_intensity(r["dilated"], raw, ty, bits)
    assert tc.same(r["texture"], g["texture"]) and tc.same(r["texture"], R.glcm(r["dilated"], raw, 64, ty, bits))
    assert r["texture"]["pairs"] > 0
    assert r["measure"] == g["measure"] and dict(r["diameters"]) == dict(g["diameters"])
    assert r["measure_json"] == g["measure_json"]
