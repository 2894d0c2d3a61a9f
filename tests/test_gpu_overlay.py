"""Colour overlay on the MI355X: the RGB JPEG encoder (k4_jpeg_rgb.hip), the overlay render
(render_overlay_kernel) and the engine's third output, against the golden model and Pillow."""
import os

import numpy as np
import pytest

from conftest import run_bin
from overlay_images import pillow_jpeg, rgb_image

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def m():
    import nm03_capstone_project_amd as mod
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return mod


# ---- encoder ------------------------------------------------------------------------------------
# [2, 48, 80, 3]: one partial workgroup (15 MCUs of 4:2:0). [2, 272, 400, 3]: 25 MCUs per row against
# 42 (4:2:0) / 85 (4:4:4) per workgroup, so workgroups start mid-row and the Y, Cb and Cr DC
# predictors all cross workgroup boundaries. [2, 512, 512, 3]: the canvas size of the exports.
ENCODER_CASES = [((48, 80), ("noise", "gradient")), ((272, 400), ("noise", "overlay")), ((512, 512), ("overlay", "black"))]


@pytest.mark.parametrize("sampling", ["420", "444"])
@pytest.mark.parametrize("shape,kinds", ENCODER_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v[0], int) else "+".join(v))
def test_jpeg_encode_rgb_matches_golden_and_pillow(m, shape, kinds, sampling):
    h, w = shape
    imgs = np.stack([rgb_image(k, h, w, seed=h + i) for i, k in enumerate(kinds)])
    assert imgs.shape == (2, h, w, 3)
    samp = {"420": 0, "444": 1}[sampling]
    out = m.ops.jpeg_encode_rgb(torch.from_numpy(imgs).cuda(), 75, True, sampling)
    assert len(out) == 2
    for i in range(2):
        assert out[i] is not None, "the default capacity holds any image"
        assert out[i] == m.native().jpeg_encode_rgb(imgs[i], 75, samp), (kinds[i], "vs golden")
        assert out[i] == pillow_jpeg(imgs[i], 75, samp), (kinds[i], "vs Pillow")


def test_jpeg_encode_rgb_capacity_and_arguments(m):
    img = torch.from_numpy(rgb_image("noise", 48, 80, seed=3)).cuda()
    full = m.ops.jpeg_encode_rgb(img, 75, False)[0]
    assert m.ops.jpeg_encode_rgb(img, 75, False, "420", out_cap=len(full) + 16)[0] == full
    assert m.ops.jpeg_encode_rgb(img, 75, False, "420", out_cap=len(full) - 16)[0] is None  # overflow is reported, never truncated
    with pytest.raises(ValueError):
        m.ops.jpeg_encode_rgb(img, 75, True, "gray")
    with pytest.raises(ValueError):
        m.ops.jpeg_encode_rgb(img[:40], 75)


# ---- render -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,spacing", [((256, 256), (1.0, 1.0)), ((200, 160), (0.9, 1.2))], ids=["exact2x", "aspect_fit"])
@pytest.mark.parametrize("nearest", [False, True], ids=["bilinear", "nearest"])
def test_render_overlay_matches_reference_and_golden(m, shape, spacing, nearest):
    n = m.native()
    h, w = shape
    raw = n.phantom_slice(h, w, 3, 12, 25, 7)
    g = n.golden_run(raw, "u16", 16, 1.0, 0.0, n.PipelineParams(), n.RenderParams(), spacing[0], spacing[1])
    dil = g["dilated"]
    brd = n.golden_border(dil, 2)
    assert dil.sum() > brd.sum() > 0
    lo, hi = g["window"]
    color = (0, 255, 0) if not nearest else (255, 0, 128)
    want = n.golden_render_overlay(raw.astype(np.float32), dil, brd, lo, hi, spacing[0], spacing[1], 512, 512, nearest, 153,
                                   255, list(color))
    if spacing != (1.0, 1.0):
        assert not want[:, 0].any() or not want[0].any(), "the aspect fit leaves black bars"
    t_raw = torch.from_numpy(raw.astype(np.int16)).cuda()
    t_dil, t_brd = torch.from_numpy(dil.astype(bool)).cuda(), torch.from_numpy(brd.astype(bool)).cuda()
    got = m.ops.render_overlay(t_raw, t_dil, t_brd, spacing=spacing, nearest=nearest, color=color)
    assert got.shape == (512, 512, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)
    ref = m.ops.reference.overlay(torch.from_numpy(raw.astype(np.float32)).cuda(), lo, hi, t_dil, t_brd, spacing=spacing,
                                  nearest=nearest, color=color)
    assert torch.equal(got, ref)
    assert (want[..., 1] != want[..., 0]).any(), "the overlay carries colour"


# ---- engine -------------------------------------------------------------------------------------
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


def _golden(native, path, cfg):
    raw, meta = native.read_slice(path)
    return native.golden_run(raw, meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"],
                             cfg.pipeline_params(), cfg.render_params(), meta["spacing_x"], meta["spacing_y"])


@pytest.fixture(scope="module")
def cohort30(tmp_path_factory, m):
    """30 slices: 6 patients × 5."""
    root = str(tmp_path_factory.mktemp("data30")) + "/"
    m.native().synth_cohort(root, patients=6, min_slices=5, max_slices=5, threads=4)
    return root


@pytest.mark.parametrize("sampling", [0, 1], ids=["420", "444"])
def test_run_array_overlay_matches_golden(m, sampling):
    n = m.native()
    raw = n.phantom_slice(256, 256, 3, 12, 25, 7)
    meta = {"type": "u16", "stored_bits": 16, "slope": 1.0, "intercept": 0.0, "spacing_x": 1.0, "spacing_y": 1.0}
    cfg = m.PipelineConfig(batch_size=1, streams=1, threads=2, overlay=True, overlay_color=(255, 200, 0),
                           jpeg_sampling=sampling)
    pipe = m.SlicePipeline(cfg)
    ref = pipe.golden(raw, meta)
    brd = n.golden_border(ref["dilated"], cfg.border_radius)
    assert brd.sum() > 0 and (ref["dilated"].astype(bool) & ~brd.astype(bool)).sum() > 0, "a colourless overlay proves nothing"
    gpu = pipe.run_array(raw, meta)
    assert np.array_equal(gpu["overlay"], ref["overlay"])
    assert gpu["jpeg_overlay"] == ref["jpeg_overlay"]
    assert len(gpu["jpegs"]) == 5
    assert gpu["jpegs"][0] == ref["jpeg_original"] and gpu["jpegs"][4] == ref["jpeg_processed"]
    plain = m.SlicePipeline(m.PipelineConfig(batch_size=1, streams=1, threads=2, jpeg_sampling=sampling)).run_array(raw, meta)
    assert "overlay" not in plain and "jpeg_overlay" not in plain and plain["jpegs"] == gpu["jpegs"]


def test_engine_cohort_overlay(m, cohort30, tmp_path):
    """Three files per slice; the overlays equal the golden model's; the two gray files are those of a
    run without the overlay; a tiny output capacity gives the same files through the host fallback;
    --resume semantics: a slice is done only when all three files exist."""
    n = m.native()
    cfg = m.PipelineConfig(batch_size=8, streams=2, threads=8, overlay=True)
    on, off, fb = str(tmp_path / "on"), str(tmp_path / "off"), str(tmp_path / "fb")
    items = _items(n, cohort30, on)
    assert len(items) == 30
    st, t = n.Engine(cfg.engine_config()).run(items)
    assert all(c == 0 for c, _ in st), st
    assert t["jpeg_fallbacks"] == 0
    st, _ = n.Engine(cfg.replace(overlay=False).engine_config()).run(_items(n, cohort30, off))
    assert all(c == 0 for c, _ in st), st
    t_on, t_off = _tree(on), _tree(off)
    assert len(t_off) == 60 and len(t_on) == 90
    assert {k: v for k, v in t_on.items() if not k.endswith("_overlay.jpg")} == t_off
    for f, od in items[::7]:
        stem = os.path.splitext(os.path.basename(f))[0]
        g = _golden(n, f, cfg)
        key = os.path.relpath(os.path.join(od, stem), on)
        assert t_on[key + "_overlay.jpg"] == g["jpeg_overlay"], key
        assert t_on[key + "_original.jpg"] == g["jpeg_original"] and t_on[key + "_processed.jpg"] == g["jpeg_processed"]
    ec = cfg.engine_config()
    ec.jpeg_out_cap = 2048
    st, t = n.Engine(ec).run(_items(n, cohort30, fb))
    assert all(c == 0 for c, _ in st), st
    assert t["jpeg_fallbacks"] == 90
    assert _tree(fb) == t_on
    # resume: only the slice whose overlay is missing is processed again
    victim = os.path.join(items[3][1], os.path.splitext(os.path.basename(items[3][0]))[0] + "_overlay.jpg")
    os.remove(victim)
    ec = cfg.replace(resume=True).engine_config()
    st, t = n.Engine(ec).run(items)
    assert [msg.startswith("resumed") for _, msg in st].count(False) == 1 and not st[3][1].startswith("resumed")
    assert _tree(on) == t_on


def test_cli_overlay_trees_identical(m, cohort_root, tmp_path):
    """--overlay in the cohort CLIs: img_processing_parallel with 1 and 2 ranks (sharing device 0) and
    img_processing_sequential write byte-identical trees of three files per slice — every file compared —
    the two gray files are those of a run without the flag, and sampled files equal the golden model."""
    n = m.native()
    env = {"NM03_DEVICE_OVERRIDE": "0", "NM03_COMM_TIMEOUT_S": "60"}
    trees = {}
    for name, tool, extra in (("par1", "img_processing_parallel", ["--overlay", "--gpus", "1", "--threads", "4"]),
                              ("par2", "img_processing_parallel", ["--overlay", "--gpus", "2", "--threads", "4"]),
                              ("seq", "img_processing_sequential", ["--overlay"]),
                              ("off", "img_processing_parallel", ["--gpus", "1", "--threads", "4"])):
        out = tmp_path / name
        r = run_bin(tool, *extra, "--data-root", cohort_root, "--out", str(out), env=env, timeout=240)
        assert r.returncode == 0, (name, r.stderr)
        trees[name] = _tree(str(out))
    items = _items(n, cohort_root, str(tmp_path / "unused"))
    assert len(trees["par1"]) == 3 * len(items) and len(trees["off"]) == 2 * len(items)
    assert trees["par2"] == trees["par1"]
    assert trees["seq"] == trees["par1"]
    assert {k: v for k, v in trees["par1"].items() if not k.endswith("_overlay.jpg")} == trees["off"]
    cfg = m.PipelineConfig(overlay=True)
    for f, od in items[::5]:
        stem = os.path.splitext(os.path.basename(f))[0]
        pid = os.path.basename(od)
        g = _golden(n, f, cfg)
        assert trees["par1"][f"{pid}/{stem}_overlay.jpg"] == g["jpeg_overlay"]
        assert trees["par1"][f"{pid}/{stem}_original.jpg"] == g["jpeg_original"]
        assert trees["par1"][f"{pid}/{stem}_processed.jpg"] == g["jpeg_processed"]


def test_test_pipeline_gpu_overlay(m, cohort_root, tmp_path):
    cpu, gpu = tmp_path / "cpu", tmp_path / "gpu"
    for out, extra in ((cpu, ["--cpu"]), (gpu, [])):
        r = run_bin("test_pipeline", *extra, "--overlay", "--data-root", cohort_root, "--out", str(out))
        assert r.returncode == 0, r.stderr
    assert (gpu / "overlay.jpg").read_bytes() == (cpu / "overlay.jpg").read_bytes()
