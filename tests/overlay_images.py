"""Test images shared by the colour-encoder tests (CPU: test_jpeg_rgb.py, GPU: test_gpu_overlay.py)."""
import io

import numpy as np


def rgb_image(kind, h, w, seed=0):
    """uint8 [h, w, 3]: noise, gradient, flat, black, or overlay-like (a gray gradient with green
    60 %-blended blobs and pure-green 2-pixel outlines — what the overlay render produces)."""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "gradient":
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)],
                        -1).astype(np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([200, 30, 120], np.uint8), (h, w, 3)).copy()
    if kind == "black":
        return np.zeros((h, w, 3), np.uint8)
    assert kind == "overlay"
    g = ((x * 3 + y * 2) * 255 // max(3 * (w - 1) + 2 * (h - 1), 1)).astype(np.int64)
    img = np.stack([g, g, g], -1)
    s = min(h, w)
    d2 = (x - w * 0.4) ** 2 + (y - h * 0.55) ** 2
    r_out, r_in = (0.3 * s) ** 2, max(0.3 * s - 2, 0) ** 2
    blob = (d2 < r_in) | (((x - w * 0.75) ** 2 + (y - h * 0.25) ** 2) < (0.1 * s) ** 2)
    ring = (d2 >= r_in) & (d2 < r_out)
    color = np.array([0, 255, 0], np.int64)
    a = 153
    img[blob] = (a * color + (255 - a) * img[blob] + 127) // 255
    img[ring] = color
    return img.astype(np.uint8)


def pillow_jpeg(rgb, quality, sampling):
    """Pillow's (libjpeg-turbo's) file for an RGB array; sampling 0 = 4:2:0, 1 = 4:4:4."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=quality, subsampling=2 if sampling == 0 else 0)
    return b.getvalue()
