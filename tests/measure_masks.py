"""Named test masks for the measurement tests (not a conftest): build(name, h, w) → bool [h, w].

The shapes are the ones a labelling kernel gets wrong: word boundaries (columns 63/64/65 and w − 1),
many tiny components (checkerboard), one component with a very long path (serpentine, spiral), ragged
components (noise at the site-percolation threshold 0.593), holes (ring, rings3) and the degenerate
masks (empty, full, one pixel in a corner)."""
import functools

import numpy as np

NOISE_P = (0.1, 0.5, 0.593, 0.9)
NAMES = (["empty", "full", "one_pixel_tl", "one_pixel_tr", "one_pixel_bl", "one_pixel_br", "checkerboard", "diag", "ring",
          "rings3", "comb", "serpentine", "serpentine_v", "spiral", "word_edges"] + [f"noise_{p}" for p in NOISE_P])


def _annulus(h, w, cy, cx, r_out, r_in):
    y, x = np.mgrid[0:h, 0:w]
    d2 = (y - cy) ** 2 + (x - cx) ** 2
    return (d2 <= r_out * r_out) & (d2 >= r_in * r_in)


def _serpentine(h, w):
    """One component: every fourth row full, joined to the next at alternating ends (path ≈ h·w/4)."""
    m = np.zeros((h, w), bool)
    m[0::4, :] = True
    for k, y in enumerate(range(0, h - 4, 4)):
        m[y + 1:y + 4, (w - 1) if k % 2 == 0 else 0] = True
    return m


def _spiral(h, w):
    """A rectangular spiral, one pixel wide with a one-pixel gap between the turns, walked inwards from
    the top-left corner: one component whose path visits about half the pixels."""
    m = np.zeros((h, w), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        return 0 <= yy < h and 0 <= xx < w and not m[yy, xx]

    def can_go(dy, dx):
        # the next cell is free, and the one after it is not an earlier turn of the spiral
        ny, nx = y + dy, x + dx
        return free(ny, nx) and (free(ny + dy, nx + dx) or not (0 <= ny + dy < h and 0 <= nx + dx < w))

    turns = 0
    while turns < 2:
        if can_go(dy, dx):
            y, x = y + dy, x + dx
            m[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy  # turn right
            turns += 1
    return m


def _word_edges(h, w):
    """Runs that start, end and cross at columns 63 / 64 / 65 and at w − 1; a second copy with blank rows between."""
    runs = [(60, 63), (64, 66), (62, 65), (63, 63), (64, 64), (65, w - 1), (0, w - 1), (w - 1, w - 1), (0, 63), (64, w - 1),
            (1, 62), (127, 128), (128, 130), (w - 2, w - 1)]
    m = np.zeros((h, w), bool)
    y = 0
    for gap in (1, 2):
        for a, b in runs:
            if y >= h:
                return m
            a, b = max(0, min(a, w - 1)), max(0, min(b, w - 1))
            if a <= b:
                m[y, a:b + 1] = True
            y += gap
    return m


@functools.lru_cache(maxsize=None)
def build(name, h, w):
    """The named mask at h × w (cached: callers get a read-only array)."""
    m = _build(name, h, w)
    m.setflags(write=False)
    return m


def _build(name, h, w):
    m = np.zeros((h, w), bool)
    if name == "empty":
        return m
    if name == "full":
        return ~m
    if name.startswith("one_pixel_"):
        m[0 if name[-2] == "t" else h - 1, 0 if name[-1] == "l" else w - 1] = True
        return m
    if name == "checkerboard":
        y, x = np.mgrid[0:h, 0:w]
        return (y + x) % 2 == 0
    if name == "diag":
        i = np.arange(min(h, w))
        m[i, i] = True
        return m
    if name == "ring":
        r = min(h, w) / 2 - 1
        return _annulus(h, w, (h - 1) / 2, (w - 1) / 2, r, r / 2)
    if name == "rings3":
        r = min(h, w) / 5
        return (_annulus(h, w, r - 1, r - 1, r, r / 2)                      # touches the frame
                | _annulus(h, w, h - r - 2, w - r - 2, r, r / 2)
                | _annulus(h, w, h / 2, w / 2, r * 0.8, r * 0.3))
    if name == "comb":
        m[0, :] = True
        m[:, 0::2] = True
        return m
    if name == "serpentine":
        return _serpentine(h, w)
    if name == "serpentine_v":
        return _serpentine(w, h).T.copy()
    if name == "spiral":
        return _spiral(h, w)
    if name == "word_edges":
        return _word_edges(h, w)
    if name.startswith("noise_"):
        p = float(name[len("noise_"):])
        return np.random.default_rng(int(p * 1000) + 7919 * h + w).random((h, w)) < p
    raise KeyError(name)


def region_of(mask):
    """A second plane for region_px: the mask without every third column."""
    r = mask.copy()
    r[:, 2::3] = False
    return r


def raw_of(h, w, seed=1):
    """16-bit samples with every bit in use (so signed and 12-bit interpretations differ from the unsigned one)."""
    return np.random.default_rng(seed * 65537 + h * 4099 + w).integers(0, 65536, size=(h, w), dtype=np.uint16)
