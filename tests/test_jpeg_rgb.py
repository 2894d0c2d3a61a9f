"""Golden colour JPEG encoder (jpeg::encode_rgb) and golden overlay render, on the CPU.

The encoder must be byte-identical to libjpeg(-turbo) as Pillow drives it: RGB → YCbCr, 4:2:0 chroma
by h2v2 downsampling, edge replication to whole MCUs, chroma quantisation and chroma Huffman tables."""
import numpy as np
import pytest

from overlay_images import pillow_jpeg, rgb_image

pytest.importorskip("PIL.Image")

SHAPES = [(512, 512), (64, 48), (100, 37), (33, 130)]
KINDS = ["noise", "gradient", "flat", "overlay"]


@pytest.mark.parametrize("sampling", [0, 1], ids=["420", "444"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_rgb_matches_pillow(native, shape, kind, sampling):
    rgb = rgb_image(kind, *shape, seed=shape[0] + shape[1])
    assert native.jpeg_encode_rgb(rgb, 75, sampling) == pillow_jpeg(rgb, 75, sampling)


@pytest.mark.parametrize("sampling", [0, 1], ids=["420", "444"])
@pytest.mark.parametrize("quality", [1, 10, 25, 50, 90, 95, 100])
def test_encode_rgb_quality_matches_pillow(native, quality, sampling):
    rgb = rgb_image("noise", 64, 64, seed=quality)
    assert native.jpeg_encode_rgb(rgb, quality, sampling) == pillow_jpeg(rgb, quality, sampling)


def test_encode_rgb_gray_sampling_raises(native):
    with pytest.raises(ValueError):
        native.jpeg_encode_rgb(rgb_image("flat", 16, 16), 75, 2)


@pytest.mark.parametrize("sampling", [0, 1], ids=["420", "444"])
@pytest.mark.parametrize("shape", [(64, 48), (100, 37)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_rgb_of_gray_equals_encode_gray(native, shape, sampling):
    """R = G = B converts to exactly (Y, 128, 128): the colour encoder then writes the gray encoder's file."""
    g = rgb_image("noise", *shape, seed=5)[..., 0].copy()
    rgb = np.stack([g, g, g], -1)
    assert native.jpeg_encode_rgb(rgb, 75, sampling) == native.jpeg_encode_gray(g, 75, sampling)


def _overlay_formula(gray, alpha, color):
    a = alpha.astype(np.int64)[..., None]
    return ((a * np.array(color, np.int64) + (255 - a) * gray.astype(np.int64)[..., None] + 127) // 255).astype(np.uint8)


@pytest.mark.parametrize("spacing,color", [((1.0, 1.0), (0, 255, 0)), ((0.9, 1.2), (255, 64, 0))])
def test_golden_overlay_is_the_blend_of_its_own_outputs(native, spacing, color):
    """golden_run's overlay canvas equals the integer blend formula evaluated on the run's own
    original render and on the label render of its dilated mask and border."""
    import io

    from PIL import Image
    raw = native.phantom_slice(200, 160, 3, 12, 25, 7)
    rp = native.RenderParams()
    assert rp.overlay is False and tuple(rp.overlay_color) == (0, 255, 0)
    rp.overlay = True
    rp.overlay_color = list(color)
    rp.jpeg_sampling = 1  # 4:4:4 files: the decoded luma is close to the canvases
    g = native.golden_run(raw, "u16", 16, 1.0, 0.0, native.PipelineParams(), rp, spacing[0], spacing[1])
    off = native.golden_run(raw, "u16", 16, 1.0, 0.0, native.PipelineParams(), native.RenderParams(), spacing[0], spacing[1])
    assert "overlay" not in off and "jpeg_overlay" not in off
    dil = g["dilated"]
    brd = native.golden_border(dil, rp.border_radius)
    assert dil.sum() > brd.sum() > 0, "the phantom slice must have fill and border pixels"
    lo, hi = g["window"]
    values = raw.astype(np.float32)
    gray = native.golden_render_gray(values, lo, hi, spacing[0], spacing[1], 512, 512, False)
    alpha = native.golden_render_labels(dil, brd, spacing[0], spacing[1], 512, 512, native.opacity_u8(rp.label_opacity),
                                        native.opacity_u8(rp.border_opacity))
    assert set(np.unique(alpha)) == {0, 153, 255}
    want = _overlay_formula(gray, alpha, color)
    assert g["overlay"].shape == (512, 512, 3) and g["overlay"].dtype == np.uint8
    assert np.array_equal(g["overlay"], want)
    assert g["jpeg_overlay"] == native.jpeg_encode_rgb(want, 75, 1)
    assert np.array_equal(native.golden_render_overlay(values, dil, brd, lo, hi, spacing[0], spacing[1], 512, 512, False,
                                                       153, 255, list(color)), want)
    # The gray outputs are the run's own: the original file decodes to the gray canvas' neighbourhood.
    dec = np.asarray(Image.open(io.BytesIO(g["jpeg_original"])).convert("L")).astype(int)
    assert np.abs(dec - gray.astype(int)).mean() < 3
    im = Image.open(io.BytesIO(g["jpeg_overlay"]))
    assert im.mode == "RGB" and im.size == (512, 512)


def test_golden_overlay_rejects_gray_sampling(native):
    rp = native.RenderParams()
    rp.overlay = True
    rp.jpeg_sampling = 2
    with pytest.raises(ValueError):
        native.golden_run(native.phantom_slice(128, 128, 3, 12, 25, 7), "u16", 16, 1.0, 0.0, native.PipelineParams(), rp)
