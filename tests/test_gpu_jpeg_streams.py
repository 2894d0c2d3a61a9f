"""GPU tests (MI355X) of the JPEG encoders (K4: k4_jpeg.hip, k4_jpeg_rgb.hip, jpeg_device.h) on streams
that take the branches noise, gradients and label canvases never do: ZRL runs, DC category 11 and AC
category 10, blocks without EOB, 0xFF across a part edge at every alignment and in the padded last
byte, exact half quotients, and both sides of the LDS range limit with the neighbours of a poisoned
image intact. Bytes only: the inputs and the walker that proves each one takes its branch are in
jpeg_stream_cases.py, and test_jpeg_stream_cases.py holds the golden encoder to libjpeg (Pillow)
for every case on the CPU.

What a broken step changes: without the ZRL loop a run above 15 indexes the wrong symbol (every
sparse_hf case, by reading); without `own += strad_v == 0xFFu` a two-part straddle image reports a
size one byte short; without `own += fin_v == 0xFFu` every final image does; without the look-back's
`++fq` the third part of a straddle3 image lands one byte early whenever it sees part 1 as an
aggregate (the last three on a host model of jpeg_emit_range's stuffing steps:
test_jpeg_stream_cases.py::test_stuffing_model_gives_the_segment_and_each_dropped_step_is_noticed)."""
import os

import numpy as np
import pytest
import torch

import jpeg_stream_cases as jc
import nm03_capstone_project_amd as nm
from nm03_capstone_project_amd import ops

pytestmark = pytest.mark.gpu

_SAMPLING = {"420": 0, "444": 1, "gray": 2}  # ops.jpeg_encode's names → jpeg::Sampling
_GRAY_LAUNCHES = jc.gray_cases()
_RGB_LAUNCHES = {s: jc.rgb_cases(s) for s in ("420", "444")}


@pytest.fixture(scope="module", autouse=True)
def _require_gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    assert nm.native().device_count() >= 1


def _encode_gray(images, quality, sampling):
    """One launch of equally shaped gray images [N, H, W]."""
    return ops.jpeg_encode(torch.from_numpy(np.stack(images)).cuda(), quality, sampling=sampling)


def _check_gray_launch(native, cases, quality, sampling, runs=1):
    names, images = list(cases), list(cases.values())
    golden = [native.jpeg_encode_gray(g, quality, _SAMPLING[sampling]) for g in images]
    for run in range(runs):
        outs = _encode_gray(images, quality, sampling)
        for name, out, want in zip(names, outs, golden):
            assert out is not None, f"{name} (run {run}): the encoder gave up on an image within its limits"
            assert out == want, f"{name} (run {run}) vs golden"


def _launch_id(key):
    q, (h, w) = key
    return f"q{q}_{h}x{w}"


@pytest.mark.parametrize("sampling", ["420", "444", "gray"])
@pytest.mark.parametrize("key", sorted(_GRAY_LAUNCHES), ids=_launch_id)
def test_gray_cases_vs_golden(native, key, sampling):
    """sparse_hf (one, two and three ZRL symbols a block, blocks without EOB, 13 % 0xFF bytes; one
    partial part and seven parts that start mid-row), dc_checker (DC differences of ±2040, category 11,
    also at a part's first block from the recomputed predecessor), binary_noise (AC category 10, blocks
    past 800 bits into the spill slots), uniform_noise (one part at 92 % of the range limit) and
    flat_levels (exact half quotients at quality 50): the cases of one quality and shape in one launch."""
    _check_gray_launch(native, _GRAY_LAUNCHES[key], key[0], sampling)


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
def test_straddle_and_final_in_one_launch(native, sampling):
    """The seven straddle images (part 1 starts at alignment 1..7 on a 0xFF byte) and the seven final
    images (the padded last byte is 0xFF with 1..7 stream bits) in one launch, run twice: the same
    golden bytes both times. Whether the last part sees its predecessor as an aggregate or as an
    inclusive record depends on timing, which the test cannot choose; both must give these bytes. (At
    4:2:0 and 4:4:4 the MCUs end in zero bits and nothing straddles: byte equality only.)"""
    _check_gray_launch(native, jc.edge_cases(), 100, sampling, runs=2)


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
def test_straddle_with_a_successor(native, sampling):
    """Three parts: the 0xFF byte across the edge of part 1 must be counted in part 2's output
    position — from part 1's inclusive record (its own straddle count), or, when part 2 sees part 1
    only as an aggregate, by the look-back's own test of the straddling byte. Twice, as above."""
    _check_gray_launch(native, jc.edge3_cases(), 100, sampling, runs=2)


@pytest.mark.parametrize("sampling", ["gray", "420", "444"])
@pytest.mark.parametrize("order", [(0, 1, 2), (1, 0, 2), (0, 2, 1)], ids=["middle", "first", "last"])
@pytest.mark.parametrize("shape", jc.LIMIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_range_limit_poisons_one_image_only(native, shape, order, sampling):
    """[uniform_noise, binary_noise, flat_levels] at 128×128 (one full part each) and [uniform_noise,
    binary_noise, straddle(3)] at 128×256 (two), quality 100, one launch each: every part of the
    binary noise exceeds the 221 120-bit LDS range and the image comes back None; the uniform noise
    (92 % of the limit) and the third image share the launch's look-back area and the round-robin
    dispatch with it and equal the golden encoder — with the poisoned image in the middle, first
    and last."""
    cases = jc.limit_launch(shape)
    names = [list(cases)[i] for i in order]
    outs = _encode_gray([cases[n] for n in names], 100, sampling)
    for name, out in zip(names, outs):
        if name == "binary_noise":
            assert out is None, "a part above the range limit must poison its image"
        else:
            assert out is not None, f"{name}: poisoned by its neighbour"
            assert out == native.jpeg_encode_gray(cases[name], 100, _SAMPLING[sampling]), f"{name} vs golden"


@pytest.mark.parametrize("sampling", ["420", "444"])
@pytest.mark.parametrize("key", sorted(_RGB_LAUNCHES["420"]), ids=_launch_id)
def test_rgb_cases_vs_golden(native, key, sampling):
    """The colour encoder on sparse_hf and binary noise per channel (ZRL runs in Y, Cb and Cr, several
    parts), a checker of saturated complements (chroma DC differences of ±2040) and one straddle and one
    final image (a Cr block without EOB before a large luma step; the padded last byte 0xFF)."""
    cases = _RGB_LAUNCHES[sampling][key]
    imgs = np.stack(list(cases.values()))
    outs = ops.jpeg_encode_rgb(torch.from_numpy(imgs).cuda(), key[0], True, sampling, out_cap=64 * 1024)
    for (name, img), out in zip(cases.items(), outs):
        assert out is not None, name
        assert out == native.jpeg_encode_rgb(img, key[0], _SAMPLING[sampling]), f"{name} vs golden"


@pytest.mark.parametrize("sampling", ["420", "444"])
@pytest.mark.parametrize("order", [(0, 1, 2), (1, 0, 2), (0, 2, 1)], ids=["middle", "first", "last"])
def test_rgb_range_limit_poisons_one_image_only(native, order, sampling):
    """The colour encoder's launch of [rgb_palette_noise, rgb_over_limit, rgb_sparse_hf] at quality 100:
    the stored image's full part exceeds the 221 120-bit LDS range (222–223 Kbit) and the image comes
    back None; the palette noise (a part at 90–94 % of the limit) and the sparse image equal the golden
    encoder — with the poisoned image in the middle, first and last. The streams are at most 32 KB of
    the 256 KiB out_cap: capacity is not what fails."""
    cases = jc.rgb_limit_launch(sampling)
    names = [list(cases)[i] for i in order]
    imgs = np.stack([cases[n] for n in names])
    outs = ops.jpeg_encode_rgb(torch.from_numpy(imgs).cuda(), 100, True, sampling, out_cap=jc.RGB_LIMIT_OUT_CAP)
    for name, out in zip(names, outs):
        if name == "rgb_over_limit":
            assert out is None, "a part above the range limit must poison its image"
        else:
            assert out is not None, f"{name}: poisoned by its neighbour"
            assert out == native.jpeg_encode_rgb(cases[name], 100, _SAMPLING[sampling]), f"{name} vs golden"


def test_engine_falls_back_for_exactly_the_poisoned_image(native, tmp_path):
    """Engine.run on three 512×512 slices into 512² canvases at quality 100: the middle slice is 0 / max
    binary noise, so every part of its original image exceeds the range limit and the engine re-encodes
    it on the CPU. Every exported file equals the golden model's, and the fallbacks are exactly the
    images whose golden stream has a part over the limit (test_jpeg_stream_cases.py counts them): not
    none, and not the phantoms that share the batch with it."""
    slices = jc.engine_slices(native)
    cfg = nm.PipelineConfig(batch_size=4, streams=1, threads=2, jpeg_quality=100)
    d, out = tmp_path / "series", tmp_path / "out"
    d.mkdir()
    out.mkdir()
    items = []
    for i, a in enumerate(slices.values(), start=1):
        (d / f"1-{i}.dcm").write_bytes(native.dicom_bytes(a))
        items.append((str(d / f"1-{i}.dcm"), str(out)))
    ec = cfg.engine_config()
    ec.jpeg_out_cap = jc.ENGINE_OUT_CAP
    st, times = native.Engine(ec).run(items)
    assert all(c == 0 for c, _ in st), st
    assert len(list(out.iterdir())) == 2 * len(items)
    for name, (f, _) in zip(slices, items):
        raw, meta = native.read_slice(f)
        g = native.golden_run(raw, meta["type"], meta["stored_bits"], meta["slope"], meta["intercept"],
                              cfg.pipeline_params(), cfg.render_params(), meta["spacing_x"], meta["spacing_y"])
        stem = os.path.splitext(os.path.basename(f))[0]
        for kind in ("original", "processed"):
            assert (out / f"{stem}_{kind}.jpg").read_bytes() == g[f"jpeg_{kind}"], (name, kind)
    assert times["jpeg_fallbacks"] == jc.ENGINE_FALLBACKS
